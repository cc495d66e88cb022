"""Attention dropout on the 16-bit MFMA kernels: `umfa::sdpa_forward_dropout` / `umfa::sdpa_backward_dropout` custom ops (fake
implementations + autograd registered, so torch.compile(fullgraph=True) keeps them as single graph nodes) and
`dropout_attention`, the differentiable entry.

The keep mask is a pure function of (query row, key, b*H + h) and a device int64[2] rng_state = {seed, offset}.
With rng_state=None `dropout_attention` draws it with torch.randint from torch's CUDA generator on the current stream: torch.manual_seed
reproduces a call, and a captured graph draws a fresh mask on every replay.  The forward saves the two words for the backward.

Scope: 4-D device fp16 / bf16 tensors, head_dim 64 / 128, equal head counts, no attn_mask, 0 < dropout_p < 1.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops

DROPOUT_HEAD_DIMS = (64, 128)
_DTYPES = (torch.float16, torch.bfloat16)


@torch.compiler.assume_constant_result
def routing_enabled() -> bool:
    """The library option sdpa_dropout (initial value from UMFA_SDPA_DROPOUT, default 0): whether the SDPA routing sends the dropout
    calls these kernels serve to them.  A constant while torch.compile traces (read when the graph is built)."""
    if not torch.cuda.is_available():  # (no device: nothing to route to -- and the library's context needs one)
        return False
    return ops.get_option("sdpa_dropout") != "0"


def served(q, k, v, attn_mask, dropout_p) -> bool:
    """Whether the dropout kernels serve this call (static: shapes, dtypes, devices)."""
    if attn_mask is not None or not (0.0 < float(dropout_p) < 1.0):
        return False
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4 or not (q.is_cuda and k.is_cuda and v.is_cuda):
        return False
    if q.dtype not in _DTYPES or k.dtype != q.dtype or v.dtype != q.dtype:
        return False
    if q.shape[0] != k.shape[0] or q.shape[1] != k.shape[1] or k.shape != v.shape or q.shape[3] != k.shape[3]:
        return False
    return q.shape[3] in DROPOUT_HEAD_DIMS and q.shape[2] > 0 and k.shape[2] > 0


def _check(q, k, v, dropout_p):
    if not served(q, k, v, None, dropout_p):
        raise ValueError("dropout_attention: needs 4-D device fp16 / bf16 tensors [B, H, S, D] with equal head counts, head_dim 64 or 128, "
                         f"and 0 < dropout_p < 1 (got {tuple(q.shape)} {q.dtype}, {tuple(k.shape)}, dropout_p={dropout_p})")


def new_rng_state(device) -> torch.Tensor:
    """{seed, offset} drawn from torch's CUDA generator on the current stream (graph-safe: a replay draws anew)."""
    return torch.randint(-(2 ** 63), 2 ** 63 - 1, (2,), dtype=torch.int64, device=device)


@torch.library.custom_op("umfa::sdpa_forward_dropout", mutates_args=(), device_types="cuda")
def sdpa_forward_dropout(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, is_causal: bool, scale: float, dropout_p: float,
                         rng_state: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """O (q's dtype) and the undropped fp32 log-sum-exp [B*H*Sq] (umfa_attention_forward_dropout_stream)."""
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    return ops.attention_forward_dropout(q, k, v, float(dropout_p), rng_state, scale=float(scale), causal=bool(is_causal))


@sdpa_forward_dropout.register_fake
def _(q, k, v, is_causal, scale, dropout_p, rng_state):
    B, H, Sq, D = q.shape
    return q.new_empty((B, H, Sq, D)), q.new_empty((B * H * Sq,), dtype=torch.float32)


@torch.library.custom_op("umfa::sdpa_backward_dropout", mutates_args=(), device_types="cuda")
def sdpa_backward_dropout(dout: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, lse: torch.Tensor,
                          is_causal: bool, scale: float, dropout_p: float,
                          rng_state: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """dQ, dK, dV in the operand dtype (umfa_attention_backward_dropout_stream), the forward's mask bit for bit."""
    return ops.attention_backward_dropout(dout.to(q.dtype).contiguous(), q.contiguous(), k.contiguous(), v.contiguous(), out.contiguous(),
                                          lse, float(dropout_p), rng_state, scale=float(scale), causal=bool(is_causal))


@sdpa_backward_dropout.register_fake
def _(dout, q, k, v, out, lse, is_causal, scale, dropout_p, rng_state):
    return torch.empty_like(q, memory_format=torch.contiguous_format), torch.empty_like(k, memory_format=torch.contiguous_format), \
        torch.empty_like(v, memory_format=torch.contiguous_format)


def _setup_context(ctx, inputs, output):
    q, k, v, is_causal, scale, dropout_p, rng_state = inputs
    out, lse = output
    ctx.save_for_backward(q, k, v, out, lse, rng_state)
    ctx.is_causal, ctx.scale, ctx.dropout_p = bool(is_causal), float(scale), float(dropout_p)


def _backward(ctx, dout, dlse):
    q, k, v, out, lse, rng_state = ctx.saved_tensors
    dq, dk, dv = torch.ops.umfa.sdpa_backward_dropout(dout, q, k, v, out, lse, ctx.is_causal, ctx.scale, ctx.dropout_p, rng_state)
    return dq, dk, dv, None, None, None, None


sdpa_forward_dropout.register_autograd(_backward, setup_context=_setup_context)


def dropout_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, dropout_p: float, *, causal: bool = False,
                      scale: Optional[float] = None, rng_state: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(q k^T scale [causal]) with attention dropout, @ v -- differentiable in q, k and v.  O = s * (keep o P) V with
    s = 1 / (1 - p) as realised.  Raises ValueError outside the kernels' scope (see the module docstring)."""
    _check(q, k, v, dropout_p)
    if rng_state is None:
        rng_state = new_rng_state(q.device)
    elif rng_state.dtype != torch.int64 or rng_state.numel() != 2 or not rng_state.is_cuda:
        raise ValueError("rng_state: a device int64 tensor of two words {seed, offset}")
    sm = float(scale) if scale is not None else float(q.shape[-1]) ** -0.5
    return torch.ops.umfa.sdpa_forward_dropout(q, k, v, bool(causal), sm, float(dropout_p), rng_state.contiguous())[0]
