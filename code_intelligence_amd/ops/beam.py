"""Beam-search selection (K11): the two per-word steps of fastai 1.x
``LanguageLearner.beam_search`` that follow the decoder.

``topk_logprobs``: per row, ``lp = log_softmax(logits)`` and the ``k`` largest
``lp`` in descending order, ties to the lower vocabulary index. ``unk_idx`` is
never returned but, as in fastai, it is part of the softmax. Selection compares
the raw logits, so the index set and order are exact for the given tensor.

``beam_select``: candidates ``s[b*k + j] = scores[b] - vals[b][j]`` (lower is
better); the ``min(beam_sz, B*k)`` smallest in ascending order, ties to the
lower flat index, with ``parent = flat // k`` and ``token = idx[flat]``.

On ROCm each is one HIP launch (beam.hip). On the CPU the same rules run in
PyTorch in the input dtype with stable sorts (fp64 inputs give a reference).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import extension as ext

__all__ = ["topk_logprobs", "beam_select", "MAX_K", "MAX_CANDIDATES"]

MAX_K = 64                  # top-k rounds per row
MAX_CANDIDATES = 16384      # B*k keys sorted in one workgroup's LDS


def topk_logprobs(logits: Tensor, k: int, unk_idx: int = -1,
                  out: Optional[Tuple[Tensor, Tensor]] = None
                  ) -> Tuple[Tensor, Tensor]:
    """logits (B,V), unit stride along V -> ``(vals (B,k), idx (B,k) int64)``.

    GPU: fp32, bf16 or fp16 logits; ``vals`` is fp32, written into ``out``
    when given (contiguous scratch). CPU: ``vals`` in the input dtype."""
    if logits.dim() != 2 or logits.size(0) < 1 or logits.size(1) < 1:
        raise ValueError("logits must be a non-empty (B, V) tensor")
    B, V = logits.shape
    if not -1 <= unk_idx < V:
        raise ValueError(f"unk_idx must be in [-1, {V}) (got {unk_idx})")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}] (got {k})")
    if k > V - (unk_idx >= 0):
        raise ValueError(f"k={k} exceeds the {V - (unk_idx >= 0)} candidates "
                         "of a row")
    if logits.is_cuda:
        lib = ext.require()
        if logits.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"unsupported logits dtype {logits.dtype}")
        if V != 1 and logits.stride(1) != 1:
            logits = logits.contiguous()
        if out is None:
            out = (torch.empty(B, k, device=logits.device, dtype=torch.float32),
                   torch.empty(B, k, device=logits.device, dtype=torch.int64))
        lib.topk_logprobs(logits, int(k), int(unk_idx), out[0], out[1])
        return out
    lse = torch.logsumexp(logits, dim=1, keepdim=True)
    keys = logits
    if unk_idx >= 0:
        keys = logits.clone()
        keys[:, unk_idx] = float("-inf")
    order = torch.sort(keys, dim=1, descending=True, stable=True).indices[:, :k]
    vals = logits.gather(1, order) - lse
    if out is not None:
        out[0].copy_(vals)
        out[1].copy_(order)
        return out
    return vals, order


def beam_select(scores: Tensor, vals: Tensor, idx: Tensor, beam_sz: int,
                out: Optional[Tuple[Tensor, Tensor, Tensor]] = None
                ) -> Tuple[Tensor, Tensor, Tensor]:
    """scores (B,), vals (B,k), idx (B,k) int64 -> ``(scores', parent, token)``,
    each ``(min(beam_sz, B*k),)``; ``parent`` and ``token`` are int64.

    ``out`` may hold 1-D views with a positive stride, e.g. the leading
    entries of a row of an ``(n_words, beam_sz)`` buffer; they must not overlap
    the inputs. GPU: fp32 scores and vals."""
    if vals.dim() != 2 or vals.numel() < 1:
        raise ValueError("vals must be a non-empty (B, k) tensor")
    B, k = vals.shape
    N = B * k
    if tuple(idx.shape) != (B, k) or idx.dtype != torch.int64:
        raise ValueError(f"idx must be int64 ({B}, {k})")
    if tuple(scores.shape) != (B,):
        raise ValueError(f"scores must be ({B},)")
    if beam_sz < 1:
        raise ValueError(f"beam_sz must be >= 1 (got {beam_sz})")
    if N > MAX_CANDIDATES:
        raise ValueError(f"B*k = {N} candidates exceed {MAX_CANDIDATES}")
    n_out = min(int(beam_sz), N)
    if out is not None:
        for t in out:
            if t.dim() != 1 or t.size(0) != n_out:
                raise ValueError(f"every output must be a ({n_out},) view")
    if vals.is_cuda:
        lib = ext.require()
        if scores.dtype != torch.float32 or vals.dtype != torch.float32:
            raise ValueError("scores and vals must be fp32 on the GPU")
        if out is None:
            dev = vals.device
            out = (torch.empty(n_out, device=dev, dtype=torch.float32),
                   torch.empty(n_out, device=dev, dtype=torch.int64),
                   torch.empty(n_out, device=dev, dtype=torch.int64))
        lib.beam_select(scores.contiguous(), vals.contiguous(),
                        idx.contiguous(), int(beam_sz), out[0], out[1], out[2])
        return out
    cand = (scores.unsqueeze(1) - vals).reshape(N)
    flat = torch.sort(cand, stable=True).indices[:n_out]
    res = (cand[flat], flat // k, idx.reshape(N)[flat])
    if out is not None:
        for dst, src in zip(out, res):
            dst.copy_(src)
        return out
    return res
