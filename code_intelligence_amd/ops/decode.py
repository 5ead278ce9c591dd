"""Decode-and-sample (K10): one generated word of the language model.

fastai 1.x ``LanguageLearner.predict`` semantics, per row:

  1. ``p = softmax(h . W^T + bias)`` at temperature 1
  2. ``no_unk``: ``p[unk] = 0``
  3. ``min_p``: entries with ``p < min_p`` are dropped, unless that would drop
     every remaining entry (fastai warns and samples unfiltered)
  4. weights ``p ** (1 / temperature)``
  5. one draw from the normalised weights

The draw is an inverse-CDF draw against a caller-supplied uniform ``u`` in
[0, 1): the first kept index, in ascending vocabulary order, whose running
weight sum exceeds ``u * total`` (the last kept index if none does). That
makes the op deterministic for a given ``u``.

On ROCm the step is two HIP launches (decode.hip): ``decode_logits`` streams
the decoder weight once for up to 8 rows, ``decode_sample`` filters and draws;
the id stays on the device. On the CPU the same rule runs in PyTorch in the
input dtype (fp64 inputs give a reference).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import extension as ext

__all__ = ["decode_logits", "sample_next", "TILE_V"]

TILE_V = 64     # vocabulary rows per (max, sum exp) partial


def _n_tiles(V: int) -> int:
    return (V + TILE_V - 1) // TILE_V


def decode_logits(h: Tensor, weight: Tensor, bias: Optional[Tensor],
                  out: Optional[Tuple[Tensor, Tensor]] = None
                  ) -> Tuple[Tensor, Tensor]:
    """h (B,H), weight (V,H), bias (V,) or None -> ``(logits, partials)``.

    ``partials`` is (B, ceil(V/64), 2): per 64-row vocabulary tile the max
    logit and ``sum exp(l - max)``. GPU: fp32 outputs, written into ``out``
    when given (scratch the caller reuses from word to word). CPU: the input
    dtype."""
    B, V = h.size(0), weight.size(0)
    if h.is_cuda:
        lib = ext.require()
        if out is None:
            out = (torch.empty(B, V, device=h.device, dtype=torch.float32),
                   torch.empty(B, _n_tiles(V), 2, device=h.device,
                               dtype=torch.float32))
        if h.size(1) != 1 and h.stride(1) != 1:
            h = h.contiguous()
        lib.decode_logits(h, weight, bias, out[0], out[1])
        return out
    logits = h @ weight.t()
    if bias is not None:
        logits = logits + bias
    NT = _n_tiles(V)
    pad = logits.new_full((B, NT * TILE_V - V), float("-inf"))
    tiles = torch.cat([logits, pad], dim=1).view(B, NT, TILE_V)
    m = tiles.max(dim=2).values
    s = torch.exp(tiles - m.unsqueeze(2)).sum(dim=2)
    return logits, torch.stack([m, s], dim=2)


def _cpu_sample(logits: Tensor, partials: Tensor, u: Tensor,
                temperature: float, min_p: float, unk: int
                ) -> Tuple[Tensor, Tensor]:
    B, V = logits.shape
    m = partials[..., 0].max(dim=1, keepdim=True).values
    se = (partials[..., 1] * torch.exp(partials[..., 0] - m)).sum(
        dim=1, keepdim=True)
    lse = m + torch.log(se)
    keep = torch.ones(B, V, dtype=torch.bool)
    if unk >= 0:
        keep[:, unk] = False
    passing = keep & (torch.exp(logits - lse) >= min_p)
    keep = torch.where(passing.any(dim=1, keepdim=True), passing, keep)
    w = torch.where(keep, torch.exp((logits - m) / temperature),
                    torch.zeros((), dtype=logits.dtype))
    cdf = w.cumsum(dim=1)
    target = u.to(logits.dtype).unsqueeze(1) * cdf[:, -1:]
    # first index whose running sum exceeds the target: always a kept entry,
    # the sum is flat across dropped ones
    idx = torch.searchsorted(cdf, target, right=True).squeeze(1)
    last_kept = V - 1 - keep.flip(1).int().argmax(dim=1)
    idx = torch.where(idx >= V, last_kept, idx)
    logp = (logits - lse).gather(1, idx.unsqueeze(1)).squeeze(1)
    return idx, logp


def sample_next(h: Tensor, weight: Tensor, bias: Optional[Tensor], u: Tensor,
                temperature: float = 1.0, min_p: Optional[float] = None,
                unk_idx: int = -1, out_ids: Optional[Tensor] = None,
                out_logp: Optional[Tensor] = None,
                scratch: Optional[Tuple[Tensor, Tensor]] = None
                ) -> Tuple[Tensor, Tensor]:
    """Sample one id per row of ``h``. Returns ``(ids int64 (B,), logp (B,))``;
    ``logp`` is the temperature-1 log-probability of the chosen id.

    ``u`` (B,) holds the uniforms. ``out_ids`` / ``out_logp`` may be strided
    (B,) views, e.g. a column of a (B, n_words) tensor; they are written in
    place and returned. ``unk_idx=-1``: no token is excluded. ``scratch`` is
    an optional ``(logits, partials)`` pair to reuse on the GPU."""
    B, V = h.size(0), weight.size(0)
    if not temperature > 0:
        raise ValueError(f"temperature must be > 0 (got {temperature})")
    mp = 0.0 if min_p is None else float(min_p)
    if not 0.0 <= mp <= 1.0:
        raise ValueError(f"min_p must be in [0, 1] (got {min_p})")
    if not -1 <= unk_idx < V:
        raise ValueError(f"unk_idx must be in [-1, {V}) (got {unk_idx})")
    if u.numel() != B:
        raise ValueError(f"u must hold one uniform per row ({B})")
    if h.is_cuda:
        lib = ext.require()
        logits, partials = decode_logits(h, weight, bias, out=scratch)
        if out_ids is None:
            out_ids = torch.empty(B, device=h.device, dtype=torch.int64)
        if out_logp is None:
            out_logp = torch.empty(B, device=h.device, dtype=torch.float32)
        u32 = u.reshape(B).to(device=h.device, dtype=torch.float32).contiguous()
        lib.decode_sample(logits, partials, u32, float(temperature), mp,
                          int(unk_idx), out_ids, out_logp)
        return out_ids, out_logp
    logits, partials = decode_logits(h, weight, bias)
    ids, logp = _cpu_sample(logits, partials, u.reshape(B), float(temperature),
                            mp, int(unk_idx))
    if out_ids is not None:
        out_ids.copy_(ids)
        ids = out_ids
    if out_logp is not None:
        out_logp.copy_(logp)
        logp = out_logp
    return ids, logp
