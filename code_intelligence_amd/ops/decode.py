"""Decode-and-sample (K10): one generated word of the language model.

fastai 1.x ``LanguageLearner.predict`` semantics, per row:

  1. ``p = softmax(h . W^T + bias)`` at temperature 1
  2. ``no_unk``: ``p[unk] = 0``
  3. ``min_p``: entries with ``p < min_p`` are dropped, unless that would drop
     every remaining entry (fastai warns and samples unfiltered)
  4. weights ``p ** (1 / temperature)``
  5. one draw from the normalised weights

Two more filters, not in fastai, sit between steps 2 and 3. With ``l`` the
logits row, ``C`` the candidates (every index but ``unk``) and
``p_v = exp(l_v - lse)`` over the whole row:

  * ``top_k``: ``t_k`` is the k-th largest of ``{l_v : v in C}``, counted with
    multiplicity; ``k >= |C|`` does not filter.
  * ``top_p`` (nucleus): ``t_p`` is the largest ``x`` in ``{l_v : v in C}``
    with ``sum_{v in C, l_v >= x} p_v >= top_p * sum_{v in C} p_v``. The mass
    is measured over all candidates, before top-k: the two cutoffs are found
    independently and intersected. Pipelines that renormalise after top-k
    keep a smaller nucleus for the same ``top_p``.
  * ``K = {v in C : l_v >= max(t_k, t_p)}``. Every entry tied with the cutoff
    logit is kept, so ``K`` can hold more than ``k`` entries; the set is a
    function of the logits alone and always holds the best candidate.
    ``top_k=1`` is greedy decoding up to exact ties; ``top_p=1.0`` is no
    filter.

``min_p`` is then applied inside ``K`` (if nothing in ``K`` passes, the draw
is from ``K``), and steps 4 and 5 run on what is left.

The draw is an inverse-CDF draw against a caller-supplied uniform ``u`` in
[0, 1): the first kept index, in ascending vocabulary order, whose running
weight sum exceeds ``u * total`` (the last kept index if none does). That
makes the op deterministic for a given ``u``.

On ROCm the step is two HIP launches (decode.hip): ``decode_logits`` streams
the decoder weight once for up to 8 rows, ``decode_sample`` filters and draws;
the id stays on the device. With ``top_k`` / ``top_p`` a third launch between
them, ``decode_cutoff``, finds ``max(t_k, t_p)`` per row. On the CPU the same rule runs in PyTorch in the
input dtype (fp64 inputs give a reference).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import extension as ext

__all__ = ["decode_logits", "decode_cutoff", "sample_next", "TILE_V"]

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


def _check_filters(top_k: Optional[int], top_p: Optional[float]
                   ) -> Tuple[int, float]:
    """Validated ``(k, top_p)`` with 0 standing for "this filter is off"."""
    k = 0
    if top_k is not None:
        k = int(top_k)
        if k != top_k or k < 1:
            raise ValueError(f"top_k must be an int >= 1 (got {top_k})")
    p = 0.0
    if top_p is not None:
        p = float(top_p)
        if not 0.0 < p <= 1.0:
            raise ValueError(f"top_p must be in (0, 1] (got {top_p})")
        if p == 1.0:
            p = 0.0
    return k, p


def _cpu_cutoff(logits: Tensor, k: int, top_p: float, unk: int) -> Tensor:
    B, V = logits.shape
    ninf = torch.full((), float("-inf"), dtype=logits.dtype)
    cut = ninf.expand(B).clone()
    n_cand = V - (1 if unk >= 0 else 0)
    if n_cand == 0 or (k == 0 and top_p == 0.0):
        return cut
    cand = logits.clone()
    if unk >= 0:
        cand = torch.cat([cand[:, :unk], cand[:, unk + 1:]], dim=1)
    srt = cand.sort(dim=1, descending=True).values
    if 1 <= k < n_cand:
        cut = srt[:, k - 1].clone()
    if top_p > 0.0:
        mass = torch.exp(srt - srt[:, :1]).cumsum(dim=1)
        # the first place, from the top, at which the running mass reaches
        # top_p of the whole: everything tied with it is kept by l >= t_p
        at = torch.searchsorted(mass, top_p * mass[:, -1:]).squeeze(1)
        t_p = srt.gather(1, at.clamp(max=n_cand - 1).unsqueeze(1)).squeeze(1)
        cut = torch.maximum(cut, t_p)
    return cut


def decode_cutoff(logits: Tensor, top_k: Optional[int] = None,
                  top_p: Optional[float] = None, unk_idx: int = -1,
                  out: Optional[Tensor] = None) -> Tensor:
    """logits (B,V) -> (B,) ``max(t_k, t_p)`` of the module docstring: the
    logit at which the top-k / nucleus set of each row ends, ``-inf`` where
    nothing filters. GPU: fp32 logits (``decode_logits``' output), one HIP
    launch, written into ``out`` when given. CPU: the input dtype."""
    k, p = _check_filters(top_k, top_p)
    B, V = logits.shape
    if not -1 <= unk_idx < V:
        raise ValueError(f"unk_idx must be in [-1, {V}) (got {unk_idx})")
    if logits.is_cuda:
        lib = ext.require()
        if out is None:
            out = torch.empty(B, device=logits.device, dtype=torch.float32)
        lib.decode_cutoff(logits, k, p, int(unk_idx), out)
        return out
    cut = _cpu_cutoff(logits, k, p, int(unk_idx))
    if out is not None:
        out.copy_(cut)
        cut = out
    return cut


def _cpu_sample(logits: Tensor, partials: Tensor, u: Tensor,
                temperature: float, min_p: float, unk: int,
                cut: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    B, V = logits.shape
    m = partials[..., 0].max(dim=1, keepdim=True).values
    se = (partials[..., 1] * torch.exp(partials[..., 0] - m)).sum(
        dim=1, keepdim=True)
    lse = m + torch.log(se)
    keep = torch.ones(B, V, dtype=torch.bool)
    if unk >= 0:
        keep[:, unk] = False
    if cut is not None:
        keep &= logits >= cut.unsqueeze(1)
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
                scratch: Optional[Tuple[Tensor, Tensor]] = None,
                top_k: Optional[int] = None, top_p: Optional[float] = None,
                cut_scratch: Optional[Tensor] = None
                ) -> Tuple[Tensor, Tensor]:
    """Sample one id per row of ``h``. Returns ``(ids int64 (B,), logp (B,))``;
    ``logp`` is the temperature-1 log-probability of the chosen id.

    ``u`` (B,) holds the uniforms. ``out_ids`` / ``out_logp`` may be strided
    (B,) views, e.g. a column of a (B, n_words) tensor; they are written in
    place and returned. ``unk_idx=-1``: no token is excluded. ``scratch`` is
    an optional ``(logits, partials)`` pair to reuse on the GPU.

    ``top_k`` (int >= 1) / ``top_p`` (in (0, 1]) restrict the draw to the
    set ``K`` of the module docstring; ``None`` (and ``top_p=1.0``) is no
    filter, and with both off the op is exactly the two launches above.
    ``cut_scratch`` is an optional fp32 (B,) buffer for the cutoff on the
    GPU."""
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
    k, tp = _check_filters(top_k, top_p)
    filtered = k > 0 or tp > 0.0
    if h.is_cuda:
        lib = ext.require()
        logits, partials = decode_logits(h, weight, bias, out=scratch)
        if out_ids is None:
            out_ids = torch.empty(B, device=h.device, dtype=torch.int64)
        if out_logp is None:
            out_logp = torch.empty(B, device=h.device, dtype=torch.float32)
        u32 = u.reshape(B).to(device=h.device, dtype=torch.float32).contiguous()
        if filtered:
            if cut_scratch is None:
                cut_scratch = torch.empty(B, device=h.device,
                                          dtype=torch.float32)
            lib.decode_cutoff(logits, k, tp, int(unk_idx), cut_scratch)
            lib.decode_sample(logits, partials, u32, float(temperature), mp,
                              int(unk_idx), out_ids, out_logp, cut_scratch)
        else:
            lib.decode_sample(logits, partials, u32, float(temperature), mp,
                              int(unk_idx), out_ids, out_logp)
        return out_ids, out_logp
    logits, partials = decode_logits(h, weight, bias)
    cut = _cpu_cutoff(logits, k, tp, int(unk_idx)) if filtered else None
    ids, logp = _cpu_sample(logits, partials, u.reshape(B), float(temperature),
                            mp, int(unk_idx), cut)
    if out_ids is not None:
        out_ids.copy_(ids)
        ids = out_ids
    if out_logp is not None:
        out_logp.copy_(logp)
        logp = out_logp
    return ids, logp
