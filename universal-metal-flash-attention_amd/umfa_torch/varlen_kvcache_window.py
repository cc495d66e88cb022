"""Sliding-window attention for packed variable-length queries over a 16-bit paged or static KV cache: the
`umfa::varlen_kvcache_window_forward` custom op, its appending form `umfa::varlen_kvcache_window_forward_append` and the rotary form
`umfa::varlen_kvcache_window_rope_forward_append` (both declare the in-place write of k_cache / v_cache), all with fake implementations,
and `varlen_kvcache_window_attention`: `varlen_kvcache_attention` with flash-attention's window_size = (left, right) -- the call a
continuous-batching server makes for layers that attend to a local window (Mistral, Gemma 2 / 3 local layers, gpt-oss).

For sequence b with L_q,b = cu_seqlens_q[b+1] - cu_seqlens_q[b] query rows, L_k,b = cache_seqlens[b] + L_q,b keys with new tokens
(cache_seqlens[b] without; clamped as varlen_kvcache_attention clamps them) and off_b = L_k,b - L_q,b, query token i of sequence b sees key
j iff j < L_k,b, j's page is in the pool and i + off_b - left <= j <= i + off_b + right; -1 leaves a side unbounded, causal sets
right = 0.  A row that sees no key gives O = 0 and LSE = -inf; rows no sequence covers are left unwritten.  Every work item sweeps only the
128-key steps its own rows' band touches and split-KV parts divide those steps, so a launch costs what its windows hold, not what the
contexts hold.  Layouts, the packed append, the clamps and the rotary embedding are varlen_kvcache_attention's
(umfa_torch/varlen_kvcache.py).

Scope: fp16 / bf16 caches, head_dim 64 / 128, capacity and max_seqlen_q below 2^30, forward only.  fp8 caches, descales and anything else
outside raise ValueError: there is no fall-back.  A window that bounds nothing calls varlen_kvcache_attention's ops, bit for bit.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from .kvcache import _check_rotary
from .varlen_kvcache import _check, _packed_view

MAX_CAPACITY = 1 << 30  # (exclusive) the C entry's bound on the capacity and on max_seqlen_q: an open side's sentinel stays inside int32

_FN = "varlen_kvcache_window_attention"


def _window(window_size, causal: bool, max_seqlen_q: int, capacity: int) -> Tuple[int, int]:
    """window_size normalised as the C entry does it: causal sets right = 0, a side that cannot bind (left >= capacity, right >=
    max_seqlen_q) is -1; a value below -1 and anything that is not a pair of ints is a ValueError"""
    try:
        left, right = (int(w) for w in window_size)
    except (TypeError, ValueError):
        raise ValueError(f"{_FN}: window_size must be a pair of ints (got {window_size!r})") from None
    if left < -1 or right < -1:
        raise ValueError(f"{_FN}: window_size values must be >= -1 (-1: unbounded), got {(left, right)}")
    if causal:
        right = 0
    if left >= capacity:
        left = -1
    if right >= max_seqlen_q:
        right = -1
    return left, right


@torch.library.custom_op("umfa::varlen_kvcache_window_forward", mutates_args=(), device_types="cuda")
def varlen_kvcache_window_forward(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cu_seqlens_q: torch.Tensor, max_seqlen_q: int,
                                  cache_seqlens: torch.Tensor, block_table: Optional[torch.Tensor], causal: bool, window_left: int,
                                  window_right: int, scale: float, num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """O [T_q, H, D] (q's dtype) and the fp32 log-sum-exp [H, T_q] (umfa_varlen_kvcache_attention_window_forward_stream)."""
    return ops.varlen_kvcache_attention_window_forward(_packed_view(q), k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q), cache_seqlens,
                                                       block_table, scale=float(scale), causal=bool(causal),
                                                       window=(int(window_left), int(window_right)), num_splits=int(num_splits))


@varlen_kvcache_window_forward.register_fake
def _(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, causal, window_left, window_right, scale, num_splits):
    Tq, H, D = q.shape
    return q.new_empty((Tq, H, D)), q.new_empty((H, Tq), dtype=torch.float32)


@torch.library.custom_op("umfa::varlen_kvcache_window_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def varlen_kvcache_window_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                         cu_seqlens_q: torch.Tensor, max_seqlen_q: int, cache_seqlens: torch.Tensor,
                                         block_table: Optional[torch.Tensor], causal: bool, window_left: int, window_right: int, scale: float,
                                         num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """varlen_kvcache_window_forward after writing k / v [T_q, H_kv, D] into k_cache / v_cache in place at cache_seqlens[b] .."""
    return ops.varlen_kvcache_attention_window_forward(_packed_view(q), k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q), cache_seqlens,
                                                       block_table, _packed_view(k), _packed_view(v), scale=float(scale), causal=bool(causal),
                                                       window=(int(window_left), int(window_right)), num_splits=int(num_splits))


@varlen_kvcache_window_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, causal, window_left, window_right, scale, num_splits):
    Tq, H, D = q.shape
    return q.new_empty((Tq, H, D)), q.new_empty((H, Tq), dtype=torch.float32)


@torch.library.custom_op("umfa::varlen_kvcache_window_rope_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def varlen_kvcache_window_rope_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                              cu_seqlens_q: torch.Tensor, max_seqlen_q: int, cache_seqlens: torch.Tensor,
                                              rotary_cos: torch.Tensor, rotary_sin: torch.Tensor, rotary_interleaved: bool,
                                              block_table: Optional[torch.Tensor], causal: bool, window_left: int, window_right: int,
                                              scale: float, num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """varlen_kvcache_window_forward_append with the rotary embedding fused into the packed append launch: row t of sequence b is rotated
    at cache_seqlens[b] + (t - cu[b]) (the queries of a non-causal call all at cache_seqlens[b]) -- the positions do not depend on the
    window."""
    return ops.varlen_kvcache_attention_window_forward(_packed_view(q), k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q), cache_seqlens,
                                                       block_table, _packed_view(k), _packed_view(v), scale=float(scale), causal=bool(causal),
                                                       window=(int(window_left), int(window_right)), num_splits=int(num_splits),
                                                       rotary_cos=rotary_cos, rotary_sin=rotary_sin,
                                                       rotary_interleaved=bool(rotary_interleaved))


@varlen_kvcache_window_rope_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cu_seqlens_q, max_seqlen_q, cache_seqlens, rotary_cos, rotary_sin, rotary_interleaved, block_table, causal,
      window_left, window_right, scale, num_splits):
    Tq, H, D = q.shape
    return q.new_empty((Tq, H, D)), q.new_empty((H, Tq), dtype=torch.float32)


# flash_attn_varlen_func / flash_attn_with_kvcache arguments this entry accepts only at their defaults (varlen_kvcache_attention's, less
# window_size)
_UNSUPPORTED = {"cache_batch_idx": None, "cache_leftpad": None, "softcap": 0.0, "alibi_slopes": None, "seqused_k": None, "dropout_p": 0.0}


def varlen_kvcache_window_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cu_seqlens_q: torch.Tensor,
                                    max_seqlen_q: int, cache_seqlens: torch.Tensor, block_table: Optional[torch.Tensor] = None,
                                    k: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None,
                                    softmax_scale: Optional[float] = None, causal: bool = False, window_size: Tuple[int, int] = (-1, -1),
                                    num_splits: int = 0, return_softmax_lse: bool = False, rotary_cos: Optional[torch.Tensor] = None,
                                    rotary_sin: Optional[torch.Tensor] = None, rotary_interleaved: bool = False, k_descale=None,
                                    v_descale=None, **unsupported):
    """varlen_kvcache_attention with flash-attention's window_size = (left, right) over a 16-bit cache: query token i of sequence b sees
    keys i + off_b - left .. i + off_b + right of its L_k,b keys, off_b = L_k,b - L_q,b; -1 leaves a side unbounded, causal sets
    right = 0.  Returns O [T_q, H, D] in q's dtype, or (O, LSE [H, T_q] fp32) with return_softmax_lse; a row that sees no key gives O = 0,
    LSE = -inf, rows no sequence covers are left unwritten.  q, cu_seqlens_q, max_seqlen_q, the caches, k / v, cache_seqlens, block_table,
    num_splits and the rotary arguments are varlen_kvcache_attention's (the rotary positions come from cache_seqlens and the causal flag,
    not from the window).  num_splits 0 sizes the split by the band.
    A window that bounds nothing -- both sides unbounded or too wide to bind (left >= capacity, right >= max_seqlen_q), or causal with an
    unbounded left -- is the varlen_kvcache_attention call, bit for bit.  fp8 caches and descales (fp8 with a window is not built),
    window values below -1 and a capacity or max_seqlen_q of 2^30 or more raise ValueError.  k_descale / v_descale are in the signature
    only to be refused by name.  cache_batch_idx / cache_leftpad / softcap / alibi_slopes / seqused_k / dropout_p are accepted at their
    defaults only."""
    for name, val in unsupported.items():
        if name not in _UNSUPPORTED:
            raise TypeError(f"{_FN}() got an unexpected keyword argument '{name}'")
        default = _UNSUPPORTED[name]
        if not (val is None if default is None else val == default):
            raise ValueError(f"{_FN}: {name} is not supported (only its default, {default!r}, is accepted)")
    if k_descale is not None or v_descale is not None:
        raise ValueError(f"{_FN}: k_descale / v_descale are not supported: fp8 caches with a window are not built (16-bit caches only)")
    if any(isinstance(t, torch.Tensor) and t.dtype == torch.float8_e4m3fn for t in (k_cache, v_cache)):
        raise ValueError(f"{_FN}: float8_e4m3fn caches are not supported: fp8 caches with a window are not built (16-bit caches only)")
    try:
        _check(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, k, v)
    except ValueError as e:  # (the packed entry's checks, under this function's name)
        raise ValueError(str(e).replace("varlen_kvcache_attention:", f"{_FN}:", 1)) from None
    cap = k_cache.shape[1] * (block_table.shape[1] if block_table is not None else 1)
    if cap >= MAX_CAPACITY or max_seqlen_q >= MAX_CAPACITY:
        raise ValueError(f"{_FN}: the cache's capacity and max_seqlen_q must be below 2^30 (got {cap}, {max_seqlen_q})")
    left, right = _window(window_size, bool(causal), int(max_seqlen_q), cap)
    sm = float(softmax_scale) if softmax_scale is not None else float(q.shape[-1]) ** -0.5
    if not sm > 0.0:
        raise ValueError(f"{_FN}: softmax_scale must be positive (got {softmax_scale})")
    rotary = _check_rotary(_FN, q, k, k is not None, rotary_cos, rotary_sin)
    mq, ns = int(max_seqlen_q), int(num_splits)
    if left < 0 and (right < 0 or (causal and right == 0)):  # nothing bound beyond causal: the unwindowed ops
        if rotary:
            out, lse = torch.ops.umfa.varlen_kvcache_rope_forward_append(q, k_cache, v_cache, k, v, cu_seqlens_q, mq, cache_seqlens, rotary_cos,
                                                                         rotary_sin, bool(rotary_interleaved), block_table, bool(causal), sm, ns)
        elif k is not None:
            out, lse = torch.ops.umfa.varlen_kvcache_forward_append(q, k_cache, v_cache, k, v, cu_seqlens_q, mq, cache_seqlens, block_table,
                                                                    bool(causal), sm, ns)
        else:
            out, lse = torch.ops.umfa.varlen_kvcache_forward(q, k_cache, v_cache, cu_seqlens_q, mq, cache_seqlens, block_table, bool(causal), sm,
                                                             ns)
    elif rotary:
        out, lse = torch.ops.umfa.varlen_kvcache_window_rope_forward_append(q, k_cache, v_cache, k, v, cu_seqlens_q, mq, cache_seqlens, rotary_cos,
                                                                            rotary_sin, bool(rotary_interleaved), block_table, bool(causal),
                                                                            left, right, sm, ns)
    elif k is not None:
        out, lse = torch.ops.umfa.varlen_kvcache_window_forward_append(q, k_cache, v_cache, k, v, cu_seqlens_q, mq, cache_seqlens, block_table,
                                                                       bool(causal), left, right, sm, ns)
    else:
        out, lse = torch.ops.umfa.varlen_kvcache_window_forward(q, k_cache, v_cache, cu_seqlens_q, mq, cache_seqlens, block_table, bool(causal),
                                                                left, right, sm, ns)
    return (out, lse) if return_softmax_lse else out
