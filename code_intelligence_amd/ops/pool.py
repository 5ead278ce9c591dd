"""Masked concat-pool (K5): cat([mean, max, last], dim=-1) with true lengths.

Reference semantics: py/code_intelligence/inference.py:93 (single sequence)
and inference.py:232-263 ``batch_seq_pool`` (batched, padding masked per true
length; "last" is the hidden state at position length-1, NOT the padded tail).

On ROCm the serve path is a single-pass HIP reduction kernel; classifier
fine-tuning goes through a second, differentiable kernel pair that also
applies fastai's MultiBatchEncoder window (keep the last ``max_len``
positions) and reads the LSTM's time-major storage in place. The CPU path is
the PyTorch composition used as the numerics reference.

Serving a fine-tuned classifier uses a third pair: ``StreamingConcatPool``
folds the encoder's chunks into a (B, 3H) fp32 ``[sum | max | last]`` state
one at a time, so no chunk outlives its encoder call, and ``pool_head``
finalises that state and runs the BatchNorm-folded two-layer head in one
launch.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import extension as ext

__all__ = ["concat_pool", "StreamingConcatPool", "pool_head"]


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


# ---- streaming pool + fused head (classifier serve path) -------------------
HEAD_LDS_BYTES = 64 * 1024


def _stream_window(lengths: Tensor, max_len: Optional[int]
                   ) -> Tuple[Tensor, Tensor]:
    """Absolute window [lo_b, len_b) of every row: len_b = max(len, 1)."""
    lens = lengths.clamp_min(1)
    lo = torch.zeros_like(lens) if not max_len else (lens - max_len).clamp_min(0)
    return lo, lens


def _finalise(state: Tensor, lengths: Tensor, max_len: Optional[int]) -> Tensor:
    """[sum | max | last] -> [sum / (len - lo) | max | last]."""
    H = state.size(1) // 3
    lo, lens = _stream_window(lengths.to(state.device), max_len)
    n = (lens - lo).to(state.dtype).unsqueeze(1)
    return torch.cat([state[:, :H] / n, state[:, H:]], dim=1)


class StreamingConcatPool:
    """Windowed concat-pool over a document that arrives in chunks.

    ``update`` folds one (B, Tc, H) chunk whose first timestep sits at
    absolute position ``t0`` into the state; ``lengths`` are whole-document
    lengths and must be the same for every chunk of one document batch. Row
    b's window is ``[max(0, len_b - max_len), len_b)`` (``max_len=None``: from
    0). The chunk may be batch-major or the transpose view of time-major
    storage, bf16 or fp32; it is read in place. On the CPU the same update
    runs in PyTorch, in ``dtype`` (fp32 by default; fp64 gives a reference).
    """

    def __init__(self, B: int, H: int, max_len: Optional[int] = None,
                 device="cpu", dtype: torch.dtype = torch.float32):
        if max_len is not None and max_len < 1:
            raise ValueError(f"max_len must be >= 1 (got {max_len})")
        self.B, self.H, self.max_len = B, H, max_len
        device = torch.device(device)
        if device.type == "cuda":
            ext.require()
            if dtype != torch.float32:
                raise ValueError("the GPU pool state is fp32")
        self.state = torch.zeros(B, 3 * H, device=device, dtype=dtype)
        self.state[:, H:2 * H] = float("-inf")
        self.lengths: Optional[Tensor] = None

    def update(self, hidden_chunk: Tensor, lengths: Tensor, t0: int) -> None:
        B, Tc, H = hidden_chunk.shape
        if (B, H) != (self.B, self.H):
            raise ValueError(f"chunk is {tuple(hidden_chunk.shape)}, pool is "
                             f"B={self.B}, H={self.H}")
        if self.state.is_cuda:
            lens32 = lengths if (lengths.dtype == torch.int32 and lengths.is_cuda
                                 and lengths.is_contiguous()) \
                else lengths.to(device=self.state.device,
                                dtype=torch.int32).contiguous()
            self.lengths = lens32
            if H != 1 and hidden_chunk.stride(2) != 1:
                hidden_chunk = hidden_chunk.contiguous()
            ext.require().concat_pool_accum(self.state, hidden_chunk, lens32,
                                            int(t0), self.max_len or 0)
            return
        self.lengths = lengths
        lo, lens = _stream_window(lengths, self.max_len)
        pos = t0 + torch.arange(Tc).unsqueeze(0)                     # (1,Tc)
        mask = ((pos >= lo.unsqueeze(1)) & (pos < lens.unsqueeze(1))).unsqueeze(-1)
        hf = hidden_chunk.to(self.state.dtype)
        hit = mask.any(dim=1)                                        # (B,1)
        # like the kernel, never touch values outside the window (a
        # non-finite pad value must not reach the sum)
        sums = self.state[:, :H] + torch.where(
            mask, hf, torch.zeros((), dtype=hf.dtype)).sum(dim=1)
        maxs = torch.maximum(
            self.state[:, H:2 * H],
            hf.masked_fill(~mask, float("-inf")).max(dim=1).values)
        tl = lens - 1 - t0
        has_last = ((tl >= 0) & (tl < Tc)).unsqueeze(1)
        last = hf[torch.arange(B), tl.clamp(0, Tc - 1)]
        self.state[:, :H] = torch.where(hit, sums, self.state[:, :H])
        self.state[:, H:2 * H] = torch.where(hit, maxs, self.state[:, H:2 * H])
        self.state[:, 2 * H:] = torch.where(has_last, last, self.state[:, 2 * H:])

    def features(self) -> Tensor:
        """(B, 3H) ``[mean, max, last]`` in the state's dtype (fp32 on a GPU)."""
        if self.lengths is None:
            raise RuntimeError("features() before any update()")
        return _finalise(self.state, self.lengths, self.max_len)


def head_fits_lds(H: int, N1: int, C: int) -> bool:
    return (3 * H + N1 + C) * 4 <= HEAD_LDS_BYTES


def pool_head(state: Tensor, lengths: Tensor, max_len: Optional[int],
              w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor,
              multi_label: bool = True) -> Tuple[Tensor, Tensor]:
    """Finalise a ``StreamingConcatPool`` state and apply the two-layer head
    ``W2 . relu(W1 . f + b1) + b2`` (eval-mode BatchNorms already folded into
    the weights). Returns ``(probs, logits)``, both (B, C): sigmoid when
    ``multi_label``, else softmax. GPU: one HIP launch, fp32. CPU: PyTorch in
    the state's dtype."""
    if state.is_cuda:
        lib = ext.require()
        lens32 = lengths.to(device=state.device, dtype=torch.int32).contiguous()
        probs, logits = lib.pool_head_fwd(state, lens32, max_len or 0,
                                          w1, b1, w2, b2, bool(multi_label))
        return probs, logits
    f = _finalise(state, lengths, max_len)
    dt = f.dtype
    h1 = torch.relu(f @ w1.to(dt).t() + b1.to(dt))
    logits = h1 @ w2.to(dt).t() + b2.to(dt)
    probs = torch.sigmoid(logits) if multi_label else torch.softmax(logits, dim=1)
    return probs, logits
