"""Fused tied-decoder softmax + cross-entropy (K6) — the FLOPs king.

Reference semantics: fastai LinearDecoder + FlattenedLoss(CrossEntropy)
over a 60k vocab (train.py:70, tie_weights/out_bias).

MI355X design: chunked over rows (CHUNK=65536 since r2 — the chunk
ladder measured 16384 -> 32768 -> 65536 at +0.3-0.5% each; ~1.05 PF for the chunk
GEMM — scripts/gemm_probe.py): per chunk one plain hipBLASLt GEMM fills a
logits tile and a HIP kernel reduces it to (logsumexp, target-logit) in a
single online pass with the decoder bias folded in (the (chunk, 60k) bias
broadcast-add never materializes).

Backward: with 288 GB of HBM3E the full (B·T, 60k) bf16 logits (~31 GB at
the bench shape) stay RESIDENT between forward and backward, so backward
skips the logits recompute GEMM entirely and transforms the saved tile in
place to dlogits = (softmax - onehot)/N (CE backward cost drops by one
full 2.5e13-FLOP GEMM per step). If the allocation does not fit
(CI_CE_SAVE_LOGITS=0 or OOM), it falls back to recompute-in-backward with
only O(B·T) state saved.

fp8 path, one-pass epilogue: when a second resident (B·T, 60k) e4m3 buffer
(~16 GB) also fits, forward's epilogue kernel reads each logits row ONCE
from registers for the logsumexp AND both dlogits forms (bf16 in place,
e4m3 copy), so backward runs no epilogue pass at all: measured 417.1 vs
422.1 ms/step (profiles/BENCH_HISTORY.md). Rows wider than the kernel's
register cache, unaligned shapes and OOM keep the two-kernel path.

Code shape: _FusedCEFunction (bf16/fp32 GEMMs) and _FusedCEFp8Function are
thin; _ce_forward and _ce_backward own the chunk loop, the resident-or-
scratch logits buffer, the recompute branch and the dW/db accumulation for
both. Per chunk they differ only in the logits GEMM (_logits_gemm), the
epilogue kernel and the dh GEMM; _fp8_chunk is the one eligibility test.

CPU path: plain F.cross_entropy composition (numerics reference)."""
from __future__ import annotations

import os

import torch
from torch import Tensor

from . import extension as ext

__all__ = ["tied_decoder_ce", "TiedDecoderCE"]

_EMPTY = {}


def _empty_f32(device) -> Tensor:
    key = str(device)
    if key not in _EMPTY:
        _EMPTY[key] = torch.empty(0, dtype=torch.float32, device=device)
    return _EMPTY[key]


def _fp8r_enabled() -> bool:
    """fp8 CE GEMMs (CI_CE_FP8R): the logits GEMM runs with OCP e4m3
    INPUTS (per-tensor scales) at the fp8 MFMA rate into the bf16-resident
    buffer, and backward's dh GEMM runs fully fp8 from an e4m3 dlogits
    scratch emitted by the dual epilogue kernel. dW stays bf16 (dlog^T is
    column-major, which _scaled_mm rejects for mat1). Measured on MI355X
    (scripts/fp8r_probe.py): fwd chunk GEMM 1.15 vs 1.59 ms, dh 0.78 vs
    1.44 ms; a fully fp8-RESIDENT buffer was tried and LOSES because the
    fp8-out GEMM epilogue is untuned (1.83 ms) and _scaled_mm ignores
    scale_result on this stack. Logits carry fp8 input-quantization error
    (~3.6% max rel, r1 probe); target logits are computed exactly via a
    bf16 gather-dot and evaluation always runs the exact bf16 path.

    DEFAULT ON since round 2: measured 601.7k vs 585.6k tokens/s at the
    bench shape with an identical 5-epoch convergence trajectory (valid
    ppl 275.03 vs 275.06, acc .2792/.2782 — profiles/BENCH_HISTORY.md).
    CI_CE_FP8R=0 restores the all-bf16 CE path."""
    return os.environ.get("CI_CE_FP8R", "1") == "1"


_STORE = 448.0  # fixed dlogits store scale: |softmax - onehot| <= 1

# ce_onepass_dual caches one bf16 row in registers: 256 threads x 32
# 16-byte vectors (ce.hip kOnepassMaxVec); wider rows take two kernels
_ONEPASS_MAX_V = 256 * 32 * 8


def _h_aug_t(lib, h: Tensor, has_bias: bool) -> Tensor:
    """(Haug, N) K-major copy of the decoder input for the dW GEMM, built
    once per backward by the pack kernel (kmajor_pack.hip).
    mm(dlog.t(), h[s:e]) hands the library a GEMM with both operands
    strided along the reduction (the chunk's rows); mm(hT[:, s:e], dlog) is
    a plain row-major one: 8.44 -> 7.20 ms per 65536-row chunk at V = 60000
    (profiles/BENCH_HISTORY.md). With a bias, row H is ones and rows
    H+1..H+15 are zero padding."""
    N, H = h.shape
    Haug = H + 16 if has_bias else H
    h_augT = torch.empty(Haug, N, dtype=h.dtype, device=h.device)
    lib.pack_kmajor(h.detach().contiguous(), h_augT, 0, 0)
    if has_bias:
        h_augT[H] = 1
        h_augT[H + 1:] = 0
    return h_augT


def _split_dw_aug_t(lib, dw_augT: Tensor, H: int, has_bias: bool):
    """fp32 (Haug, V) sums -> dw (V, H) contiguous fp32, db (V,) or None."""
    dw = torch.empty(dw_augT.shape[1], H, dtype=dw_augT.dtype,
                     device=dw_augT.device)
    lib.pack_kmajor(dw_augT[:H], dw, 0, 0)
    return dw, (dw_augT[H] if has_bias else None)


def _fp8_chunk(rows: int, H: int, V: int) -> bool:
    """Whether a chunk of `rows` rows takes the fp8 GEMMs (_scaled_mm wants
    every dimension a multiple of 16); tail and odd shapes take bf16 ones.
    Forward, the one-pass decision and backward all ask here: lse belongs
    to the logits of ONE GEMM, so they must agree chunk by chunk."""
    return rows % 16 == 0 and H % 16 == 0 and V % 16 == 0


def _logits_gemm(out: Tensor, h: Tensor, weight: Tensor, q, s: int, e: int):
    """out <- h[s:e] @ weight^T. q = (h8, w8, sa, sw), the e4m3 operands and
    their scales, or None for the all-bf16 path."""
    if q is not None and _fp8_chunk(e - s, h.shape[1], weight.shape[0]):
        h8, w8, sa, sw = q
        # w8.t(): (H, V) column-major view for mat2
        torch._scaled_mm(h8[s:e], w8.t(), scale_a=sa, scale_b=sw,
                         out_dtype=h.dtype, out=out)
    else:
        torch.mm(h[s:e], weight.t(), out=out)


def _try_empty(*shape, dtype, device):
    try:
        return torch.empty(*shape, dtype=dtype, device=device)
    except torch.cuda.OutOfMemoryError:
        return None


def _ce_forward(ctx, h: Tensor, weight: Tensor, bias, targets: Tensor,
                fp8: bool) -> Tensor:
    """Chunked forward of both autograd Functions; fp8 picks the GEMMs and
    the one-pass epilogue (see _fp8r_enabled and the module docstring)."""
    lib = ext.require()
    f8 = torch.float8_e4m3fn
    N, H = h.shape
    V = weight.shape[0]
    C = int(os.environ.get("CI_CE_CHUNK", _FusedCEFunction.CHUNK))
    dev = h.device
    lse = torch.empty(N, dtype=torch.float32, device=dev)
    tgt_logit = torch.empty(N, dtype=torch.float32, device=dev)
    b32 = bias.to(torch.float32) if bias is not None else _empty_f32(dev)
    tgt64 = targets.to(torch.int64)
    q = None
    if fp8:
        sa = (h.detach().abs().amax().float() / 448.0).clamp_min(1e-12)
        sw = (weight.detach().abs().amax().float() / 448.0).clamp_min(1e-12)
        # one-pass quantize kernel (the eager mul+clamp+cast chain is
        # three kernels and 3x the traffic — fp8util.hip)
        h8 = torch.empty(h.shape, dtype=f8, device=dev)
        lib.quantize_e4m3(h.detach().contiguous(), h8, sa)
        w8 = torch.empty(weight.shape, dtype=f8, device=dev)
        lib.quantize_e4m3(weight.detach().contiguous(), w8, sw)
        q = (h8, w8, sa, sw)
    logits_full = None
    if os.environ.get("CI_CE_SAVE_LOGITS", "1") != "0":
        logits_full = _try_empty(N, V, dtype=h.dtype, device=dev)
    # one-pass epilogue: with a second resident (N, V) e4m3 buffer the
    # row is read ONCE here (lse + both dlogits forms, scaled 1/N) and
    # backward runs no epilogue at all. Needs every chunk on the fp8
    # GEMM path and the row within the kernel's register cache.
    dlog8_full = None
    if fp8 and logits_full is not None and V <= _ONEPASS_MAX_V \
            and all(_fp8_chunk(min(N, s + C) - s, H, V)
                    for s in range(0, N, C)):
        dlog8_full = _try_empty(N, V, dtype=f8, device=dev)
    onepass = dlog8_full is not None
    if onepass:
        inv_n = (torch.ones((), dtype=torch.float32, device=dev)
                 / N).reshape(1)
    scratch = None if logits_full is not None else \
        torch.empty(min(C, N), V, dtype=h.dtype, device=dev)
    for s in range(0, N, C):
        e = min(N, s + C)
        logits = logits_full[s:e] if logits_full is not None \
            else scratch[: e - s]
        _logits_gemm(logits, h, weight, q, s, e)
        if onepass:
            # logits <- bf16((softmax-onehot)/N) in place,
            # dlog8_full <- e4m3((softmax-onehot)*448), lse out
            lib.ce_onepass_dual(logits, tgt64[s:e], b32, lse[s:e],
                                inv_n, dlog8_full[s:e], _STORE)
        else:
            lib.ce_rowstats(logits, tgt64[s:e], b32, lse[s:e],
                            tgt_logit[s:e])
    if fp8:
        # exact target logits (bf16 gather-dot, fp32 accumulation): the
        # loss value must not carry fp8 input-quantization target error
        wrows = weight.detach()[tgt64]
        tgt_logit = (h.detach() * wrows).sum(dim=1, dtype=torch.float32)
        if bias is not None:
            tgt_logit = tgt_logit + b32[tgt64]
        # the recompute fallback must rebuild each chunk's logits with the
        # GEMM that produced them here (lse belongs to THOSE logits), so it
        # keeps the e4m3 activations: O(N*H) bytes
        q = (h8 if logits_full is None else None, w8, sa, sw)
    loss = (lse - tgt_logit).mean()
    ctx.save_for_backward(h, weight, b32, tgt64, lse)
    ctx.logits_full = logits_full
    ctx.dlog8_full = dlog8_full
    ctx.q = q
    # backward walks forward's chunks: which GEMM a chunk takes depends on
    # its size
    ctx.chunk = C
    ctx.has_bias = bias is not None
    ctx.bias_dtype = bias.dtype if bias is not None else None
    return loss


def _ce_backward(ctx, dloss: Tensor):
    lib = ext.require()
    h, weight, b32, targets, lse = ctx.saved_tensors
    # logits_full: forward's logits, or after the one-pass epilogue already
    # bf16 (softmax-onehot)/N with dlog8_full its e4m3*448 copy
    logits_full, dlog8_full, q = ctx.logits_full, ctx.dlog8_full, ctx.q
    ctx.logits_full = ctx.dlog8_full = ctx.q = None  # release asap
    fp8 = q is not None
    onepass = dlog8_full is not None
    has_bias = ctx.has_bias
    N, H = h.shape
    V = weight.shape[0]
    C = ctx.chunk
    dev = h.device
    dh = torch.empty_like(h)
    scale = (dloss / N).to(torch.float32).reshape(1)
    if fp8:
        _, w8, _, sw = q
        sc_over_store = (scale.reshape(()) / _STORE)
        scratch8 = None if onepass else \
            torch.empty(min(C, N), V, dtype=torch.float8_e4m3fn, device=dev)
        # (V, H) column-major e4m3 weight for the fp8 dh GEMM
        w8_cm = w8.t().contiguous().t()
    # db folded into the dW GEMM: h^T gains a 16-row pad whose first
    # extra row is ones, so row H of dW_aug^T IS sum(dlog) — the
    # separate db reduction re-read the whole dlog chunk (7.9 GB at
    # the bench shape); 16 (not 1) keeps the GEMM M%16 alignment
    h_augT = _h_aug_t(lib, h, has_bias)
    dw_augT = torch.zeros(h_augT.shape[0], V, dtype=torch.float32,
                          device=dev)
    recompute = None if logits_full is not None else \
        torch.empty(min(C, N), V, dtype=h.dtype, device=dev)
    for s in range(0, N, C):
        e = min(N, s + C)
        c = e - s
        if logits_full is not None:
            dlog = logits_full[s:e]
        else:
            # same GEMM as forward's for this chunk: a bf16 recompute
            # of fp8-GEMM logits would not match the saved lse
            dlog = recompute[:c]
            _logits_gemm(dlog, h, weight, q, s, e)
        if onepass:
            dlog8 = dlog8_full[s:e]
        elif fp8:
            # dlog <- bf16((softmax-onehot)*dloss/N) in place;
            # scratch8 <- e4m3((softmax-onehot)*448) in the same read
            lib.ce_dlogits_dual(dlog, targets[s:e], b32, lse[s:e], scale,
                                scratch8, _STORE)
            dlog8 = scratch8[:c]
        else:
            # in place: dlog <- (softmax(dlog + bias) - onehot) * scale
            lib.ce_dlogits(dlog, targets[s:e], b32, lse[s:e], scale)
        if fp8 and _fp8_chunk(c, H, V):
            torch._scaled_mm(dlog8, w8_cm, scale_a=sc_over_store,
                             scale_b=sw, out_dtype=h.dtype, out=dh[s:e])
        else:
            torch.mm(dlog, weight, out=dh[s:e])
        dw_augT += torch.mm(h_augT[:, s:e], dlog)
    dw, db = _split_dw_aug_t(lib, dw_augT, H, has_bias)
    if onepass:
        # the stored bf16 dlogits carry 1/N, not dloss/N: apply dloss
        # to the fp32 sums inside the casts that run anyway (x*1 is
        # exact, so dloss == 1 reproduces the two-kernel path's bits)
        dl = dloss.to(torch.float32)
        dw_out = torch.empty(V, H, dtype=weight.dtype, device=dev)
        torch.mul(dw, dl, out=dw_out)
        return (dh, dw_out,
                (db * dl).to(ctx.bias_dtype) if has_bias else None, None)
    return (dh, dw.to(weight.dtype),
            db.to(ctx.bias_dtype) if has_bias else None, None)


class _FusedCEFp8Function(torch.autograd.Function):
    """fp8-GEMM variant of the fused tied-decoder CE (see _fp8r_enabled).
    Loss/grad parity vs the bf16 path is locked by
    tests/test_gpu_kernels.py (loss <2%, grad cosine >0.98), every
    sub-path vs fp64 by tests/test_gpu_ce.py, and convergence by the
    markov check in profiles/BENCH_HISTORY.md."""

    @staticmethod
    def forward(ctx, h: Tensor, weight: Tensor, bias: Tensor, targets: Tensor):
        return _ce_forward(ctx, h, weight, bias, targets, fp8=True)

    @staticmethod
    def backward(ctx, dloss: Tensor):
        return _ce_backward(ctx, dloss)


class _FusedCEFunction(torch.autograd.Function):
    CHUNK = int(os.environ.get("CI_CE_CHUNK", "65536"))

    @staticmethod
    def forward(ctx, h: Tensor, weight: Tensor, bias: Tensor, targets: Tensor):
        return _ce_forward(ctx, h, weight, bias, targets, fp8=False)

    @staticmethod
    def backward(ctx, dloss: Tensor):
        return _ce_backward(ctx, dloss)


@torch.no_grad()
def tied_decoder_accuracy(h: Tensor, weight: Tensor, bias: Tensor | None,
                          targets: Tensor, chunk: int = 16384) -> Tensor:
    """Top-1 next-token accuracy (eval metric; fastai reports accuracy
    during fit). Chunked so the (N, 60k) logits never fully materialize."""
    h2 = h.reshape(-1, h.shape[-1])
    t2 = targets.reshape(-1)
    w_t = weight.t()
    correct = torch.zeros((), dtype=torch.long, device=h.device)
    for s in range(0, h2.shape[0], chunk):
        e = min(h2.shape[0], s + chunk)
        logits = torch.mm(h2[s:e], w_t)
        if bias is not None:
            logits += bias
        correct += (logits.argmax(dim=1) == t2[s:e]).sum()
    return correct.float() / max(1, h2.shape[0])


def tied_decoder_ce(h: Tensor, weight: Tensor, bias: Tensor | None,
                    targets: Tensor) -> Tensor:
    """h: (N, H) decoder input (already output-dropped); weight: (V, H) tied
    embedding; targets: (N,) int64. Returns scalar mean CE loss."""
    if h.is_cuda:
        # fp8-resident only for TRAINING steps: evaluation (valid ppl) and
        # any no-grad loss stays exact bf16, like fp8 training recipes
        # that keep the eval loss in high precision.
        if _fp8r_enabled() and h.dtype == torch.bfloat16 \
                and torch.is_grad_enabled() and h.requires_grad:
            return _FusedCEFp8Function.apply(h, weight, bias, targets)
        return _FusedCEFunction.apply(h, weight, bias, targets)
    logits = torch.nn.functional.linear(h.float(), weight.float(),
                                        bias.float() if bias is not None else None)
    return torch.nn.functional.cross_entropy(logits, targets)


class TiedDecoderCE(torch.nn.Module):
    """Loss module bound to a LinearDecoder's weight/bias."""

    def __init__(self, decoder: torch.nn.Linear):
        super().__init__()
        self.decoder = decoder

    def forward(self, h: Tensor, targets: Tensor) -> Tensor:
        return tied_decoder_ce(h.reshape(-1, h.shape[-1]), self.decoder.weight,
                               self.decoder.bias, targets.reshape(-1))
