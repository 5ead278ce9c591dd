"""Masked concat-pool (K5): cat([mean, max, last], dim=-1) with true lengths.

Reference semantics: py/code_intelligence/inference.py:93 (single sequence)
and inference.py:232-263 ``batch_seq_pool`` (batched, padding masked per true
length; "last" is the hidden state at position length-1, NOT the padded tail).

On ROCm the serve path is a single-pass HIP reduction kernel; classifier
fine-tuning goes through a second, differentiable kernel pair that also
applies fastai's MultiBatchEncoder window (keep the last ``max_len``
positions) and reads the LSTM's time-major storage in place. The CPU path is
the PyTorch composition used as the numerics reference.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import extension as ext

__all__ = ["concat_pool"]


def _cpu_concat_pool(hidden: Tensor, lengths: Tensor,
                     max_len: Optional[int] = None) -> Tensor:
    """hidden: (B, T, H) final-layer hidden states; lengths: (B,) int64.
    With ``max_len`` row b is pooled over [max(0, len_b - max_len), len_b),
    len_b clamped to [1, T]."""
    B, T, H = hidden.shape
    ar = torch.arange(T, device=hidden.device).unsqueeze(0)          # (1,T)
    if max_len is None:
        mask = (ar < lengths.unsqueeze(1)).unsqueeze(-1)             # (B,T,1)
        count = lengths.clamp_min(1)
        last_t = (lengths - 1).clamp_min(0)
    else:
        lens = lengths.clamp(1, T)
        lo = (lens - max_len).clamp_min(0)
        mask = ((ar >= lo.unsqueeze(1)) & (ar < lens.unsqueeze(1))).unsqueeze(-1)
        count = lens - lo
        last_t = lens - 1
    # dense batch-major: the reference's sums (and its backward's) then do
    # not depend on the caller's memory layout (no-op when already dense)
    hf = hidden.float().contiguous()
    summed = (hf * mask).sum(dim=1)
    mean = summed / count.unsqueeze(1).float()
    neg = torch.finfo(torch.float32).min
    maxed = hf.masked_fill(~mask, neg).max(dim=1).values
    last = hf[torch.arange(B, device=hidden.device), last_t]
    return torch.cat([mean, maxed, last], dim=1).to(hidden.dtype)


class _ConcatPoolFunction(torch.autograd.Function):
    """GPU path with a backward: one forward kernel that also records the
    argmax (first index on ties), one backward kernel that writes every
    element of dhidden exactly once, in the input's own layout."""

    @staticmethod
    def forward(ctx, hidden: Tensor, lengths: Tensor, max_len: int):
        lib = ext.require()
        if hidden.size(2) != 1 and hidden.stride(2) != 1:
            hidden = hidden.contiguous()
        out, argmax = lib.concat_pool_fwd_idx(hidden, lengths, max_len)
        # hidden is kept only as the layout/dtype template of dhidden
        ctx.save_for_backward(argmax, lengths, hidden)
        ctx.max_len = max_len
        return out

    @staticmethod
    def backward(ctx, dout: Tensor):
        argmax, lengths, hidden = ctx.saved_tensors
        dh = ext.require().concat_pool_bwd(
            dout.contiguous(), argmax, lengths, ctx.max_len, hidden)
        return dh, None, None


def concat_pool(hidden: Tensor, lengths: Tensor,
                max_len: Optional[int] = None) -> Tensor:
    """Returns (B, 3H): [mean, max, last] pooled over true lengths; with
    ``max_len`` only over each row's last ``max_len`` valid positions.

    ``hidden`` may be any (B,T,H) tensor with unit stride along H; the
    (B,T,H) transpose view of time-major (T,B,H) storage is read without a
    copy and its gradient comes back in the same layout."""
    if max_len is not None and max_len < 1:
        raise ValueError(f"max_len must be >= 1 (got {max_len})")
    if hidden.is_cuda:
        lib = ext.require()
        lens32 = lengths.to(torch.int32).contiguous()
        needs_grad = torch.is_grad_enabled() and hidden.requires_grad
        if needs_grad or max_len is not None:
            return _ConcatPoolFunction.apply(hidden, lens32, max_len or 0)
        return lib.concat_pool(hidden.contiguous(), lens32)
    return _cpu_concat_pool(hidden, lengths, max_len)
