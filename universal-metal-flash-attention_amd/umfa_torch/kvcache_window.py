"""Sliding-window attention over a 16-bit paged or static KV cache: the `umfa::kvcache_window_forward` custom
op, its appending form `umfa::kvcache_window_forward_append` and the rotary form `umfa::kvcache_window_rope_forward_append` (both declare
the in-place write of k_cache / v_cache), all with fake implementations, and `kvcache_window_attention`: `kvcache_attention` with
flash-attention's window_size = (left, right).

With L_k = cache_seqlens[b] + S_new (clamped as kvcache_attention clamps it) and off = L_k - Sq, query token i of sequence b sees key j
iff j < L_k, j's page is in the pool and i + off - left <= j <= i + off + right; -1 leaves a side unbounded, causal sets right = 0.  A
row that sees no key gives O = 0 and LSE = -inf.  The kernel sweeps only the 128-key steps the band touches and split-KV parts divide
those steps, so a decode step costs what its window holds, not what the context holds.  Layouts, the append, the clamps and the rotary
embedding are kvcache_attention's (umfa_torch/kvcache.py).

Scope: fp16 / bf16 caches, head_dim 64 / 128, capacity below 2^30, forward only.  fp8 caches, descales and anything else outside raise
ValueError: there is no fall-back.  A window that bounds nothing calls kvcache_attention's ops, bit for bit.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from .kvcache import _check, _check_rotary, _kernel_view

MAX_CAPACITY = 1 << 30  # (exclusive) the C entry's bound: an open side's sentinel stays inside int32


def _window(window_size, causal: bool, Sq: int, capacity: int) -> Tuple[int, int]:
    """window_size normalised as the C entry does it: causal sets right = 0, a side that cannot bind (left >= capacity, right >= Sq) is
    -1; a value below -1 and anything that is not a pair of ints is a ValueError"""
    try:
        left, right = (int(w) for w in window_size)
    except (TypeError, ValueError):
        raise ValueError(f"kvcache_window_attention: window_size must be a pair of ints (got {window_size!r})") from None
    if left < -1 or right < -1:
        raise ValueError(f"kvcache_window_attention: window_size values must be >= -1 (-1: unbounded), got {(left, right)}")
    if causal:
        right = 0
    if left >= capacity:
        left = -1
    if right >= Sq:
        right = -1
    return left, right


@torch.library.custom_op("umfa::kvcache_window_forward", mutates_args=(), device_types="cuda")
def kvcache_window_forward(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_seqlens: torch.Tensor,
                           block_table: Optional[torch.Tensor], causal: bool, window_left: int, window_right: int, scale: float,
                           num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """O [B, Sq, H, D] (q's dtype) and the fp32 log-sum-exp [B, H, Sq] (umfa_kvcache_attention_window_forward_stream)."""
    return ops.kvcache_attention_window_forward(_kernel_view(q), k_cache, v_cache, cache_seqlens, block_table, scale=float(scale),
                                                causal=bool(causal), window=(int(window_left), int(window_right)), num_splits=int(num_splits))


@kvcache_window_forward.register_fake
def _(q, k_cache, v_cache, cache_seqlens, block_table, causal, window_left, window_right, scale, num_splits):
    B, Sq, H, D = q.shape
    return q.new_empty((B, Sq, H, D)), q.new_empty((B, H, Sq), dtype=torch.float32)


@torch.library.custom_op("umfa::kvcache_window_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def kvcache_window_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                  cache_seqlens: torch.Tensor, block_table: Optional[torch.Tensor], causal: bool, window_left: int,
                                  window_right: int, scale: float, num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """kvcache_window_forward after writing k / v [B, S_new, H_kv, D] into k_cache / v_cache in place at cache_seqlens[b] .."""
    return ops.kvcache_attention_window_forward(_kernel_view(q), k_cache, v_cache, cache_seqlens, block_table, _kernel_view(k), _kernel_view(v),
                                                scale=float(scale), causal=bool(causal), window=(int(window_left), int(window_right)),
                                                num_splits=int(num_splits))


@kvcache_window_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cache_seqlens, block_table, causal, window_left, window_right, scale, num_splits):
    B, Sq, H, D = q.shape
    return q.new_empty((B, Sq, H, D)), q.new_empty((B, H, Sq), dtype=torch.float32)


@torch.library.custom_op("umfa::kvcache_window_rope_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def kvcache_window_rope_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                       cache_seqlens: torch.Tensor, rotary_cos: torch.Tensor, rotary_sin: torch.Tensor,
                                       rotary_interleaved: bool, block_table: Optional[torch.Tensor], causal: bool, window_left: int,
                                       window_right: int, scale: float, num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """kvcache_window_forward_append with the rotary embedding fused into the append launch: k is rotated at cache_seqlens[b] + t on its
    way into k_cache, q at cache_seqlens[b] + i (causal) or cache_seqlens[b] (not) -- the positions do not depend on the window."""
    return ops.kvcache_attention_window_forward(_kernel_view(q), k_cache, v_cache, cache_seqlens, block_table, _kernel_view(k), _kernel_view(v),
                                                scale=float(scale), causal=bool(causal), window=(int(window_left), int(window_right)),
                                                num_splits=int(num_splits), rotary_cos=rotary_cos, rotary_sin=rotary_sin,
                                                rotary_interleaved=bool(rotary_interleaved))


@kvcache_window_rope_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cache_seqlens, rotary_cos, rotary_sin, rotary_interleaved, block_table, causal, window_left, window_right,
      scale, num_splits):
    B, Sq, H, D = q.shape
    return q.new_empty((B, Sq, H, D)), q.new_empty((B, H, Sq), dtype=torch.float32)


def kvcache_window_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: Optional[torch.Tensor] = None,
                             v: Optional[torch.Tensor] = None, cache_seqlens=None, block_table: Optional[torch.Tensor] = None,
                             softmax_scale: Optional[float] = None, causal: bool = False, window_size: Tuple[int, int] = (-1, -1),
                             num_splits: int = 0, return_softmax_lse: bool = False, rotary_cos: Optional[torch.Tensor] = None,
                             rotary_sin: Optional[torch.Tensor] = None, rotary_interleaved: bool = False, k_descale=None, v_descale=None):
    """kvcache_attention with flash-attention's window_size = (left, right) over a 16-bit cache: query token i of sequence b sees keys
    i + off - left .. i + off + right of its L_k = cache_seqlens[b] + S_new keys, off = L_k - Sq; -1 leaves a side unbounded, causal sets
    right = 0.  Returns O [B, Sq, H, D] in q's dtype, or (O, LSE [B, H, Sq] fp32) with return_softmax_lse; a row that sees no key gives
    O = 0, LSE = -inf.  q, the caches, k / v, cache_seqlens, block_table, num_splits and the rotary arguments are kvcache_attention's (the
    rotary positions come from cache_seqlens and the causal flag, not from the window).  num_splits 0 sizes the split by the band.
    A window that bounds nothing -- both sides unbounded or too wide to bind, or causal with an unbounded left -- is the kvcache_attention
    call, bit for bit.  fp8 caches and descales, window values below -1 and a capacity of 2^30 keys or more raise ValueError.
    k_descale / v_descale are in the signature only to be refused by name: code written for kvcache_attention's fp8 caches gets a
    ValueError that says so, not a TypeError about an unexpected keyword."""
    if k_descale is not None or v_descale is not None:
        raise ValueError("kvcache_window_attention: k_descale / v_descale are not supported (16-bit caches only)")
    if any(isinstance(t, torch.Tensor) and t.dtype == torch.float8_e4m3fn for t in (k_cache, v_cache)):
        raise ValueError("kvcache_window_attention: float8_e4m3fn caches are not supported with a window (16-bit caches only)")
    paged = isinstance(block_table, torch.Tensor) and block_table.dim() == 2
    if cache_seqlens is None and isinstance(k_cache, torch.Tensor) and k_cache.dim() == 4:
        cache_seqlens = k_cache.shape[1] * (block_table.shape[1] if paged else 1)  # the whole capacity
    if isinstance(cache_seqlens, int) and isinstance(q, torch.Tensor) and q.dim() == 4:
        cache_seqlens = torch.full((q.shape[0],), cache_seqlens, dtype=torch.int32, device=q.device)
    if not isinstance(cache_seqlens, torch.Tensor):
        raise ValueError("kvcache_window_attention: cache_seqlens must be an int, or a device int32 [batch] tensor")
    _check(q, k_cache, v_cache, k, v, cache_seqlens, block_table, fn="kvcache_window_attention")
    cap = k_cache.shape[1] * (block_table.shape[1] if block_table is not None else 1)
    if cap >= MAX_CAPACITY:
        raise ValueError(f"kvcache_window_attention: the cache's capacity must be below 2^30 keys per sequence (got {cap})")
    left, right = _window(window_size, bool(causal), q.shape[1], cap)
    new_tokens = k is not None and k.shape[1] > 0
    rotary = _check_rotary("kvcache_window_attention", q, k, new_tokens, rotary_cos, rotary_sin)
    sm = float(softmax_scale) if softmax_scale is not None else float(q.shape[-1]) ** -0.5
    if left < 0 and (right < 0 or (causal and right == 0)):  # nothing bound beyond causal: the unwindowed ops
        if rotary:
            out, lse = torch.ops.umfa.kvcache_rope_forward_append(q, k_cache, v_cache, k, v, cache_seqlens, rotary_cos, rotary_sin,
                                                                  bool(rotary_interleaved), block_table, bool(causal), sm, int(num_splits))
        elif new_tokens:
            out, lse = torch.ops.umfa.kvcache_forward_append(q, k_cache, v_cache, k, v, cache_seqlens, block_table, bool(causal), sm,
                                                             int(num_splits))
        else:
            out, lse = torch.ops.umfa.kvcache_forward(q, k_cache, v_cache, cache_seqlens, block_table, bool(causal), sm, int(num_splits))
    elif rotary:
        out, lse = torch.ops.umfa.kvcache_window_rope_forward_append(q, k_cache, v_cache, k, v, cache_seqlens, rotary_cos, rotary_sin,
                                                                     bool(rotary_interleaved), block_table, bool(causal), left, right, sm,
                                                                     int(num_splits))
    elif new_tokens:
        out, lse = torch.ops.umfa.kvcache_window_forward_append(q, k_cache, v_cache, k, v, cache_seqlens, block_table, bool(causal), left,
                                                                right, sm, int(num_splits))
    else:
        out, lse = torch.ops.umfa.kvcache_window_forward(q, k_cache, v_cache, cache_seqlens, block_table, bool(causal), left, right, sm,
                                                         int(num_splits))
    return (out, lse) if return_softmax_lse else out
