"""Fused LSTM layer op.

Forward over a whole (B, T, In) sequence for ONE layer:

  * the input-side projection ``x @ W_ih^T + b`` has no time dependency and
    runs as one large plain GEMM (hipBLASLt via torch.mm — per the MI355X
    design rules, library GEMMs are allowed for plain GEMMs);
  * the recurrent part is the hot sequential loop: per timestep a
    (B,H)x(H,4H) GEMM + gate activations + c/h update. On ROCm this is a
    hand-written CDNA4 kernel — either the fully fused MFMA cell kernel
    (lstm_gemm.hip) or a hipBLASLt GEMM + pointwise HIP kernel
    (lstm_pointwise.hip), selected by CI_LSTM_MODE=fused|lib.

Internally everything is TIME-MAJOR (T, B, ·): every per-step slice
(h_prev, xp_t, dgates_t) is then a contiguous (B, ·) block, which is what
both the hand-written kernels and hipBLASLt want (measured: strided
batch-major A costs the backward dh GEMM ~40% — scripts/gemm_probe.py).
The public API stays batch-first; the layer boundary transposes, and when
the neighbouring layer also runs time-major the transposes cancel into
no-op views.

Backward mirrors forward: a sequential per-timestep pointwise+GEMM loop
for dh/dc/dgates (NT layout via one weight transpose), then batched plain
GEMMs for dW_ih, dW_hh, db, dx.

Gate order follows PyTorch/cuDNN (i, f, g, o) for checkpoint parity.
The CPU path is a straightforward PyTorch reference (tests compare the
HIP kernels against it in fp32)."""
from __future__ import annotations

import os
from typing import Tuple

import torch
from torch import Tensor

from . import extension as ext

__all__ = ["lstm_forward", "sync_dw_stream"]

_side_stream = None


def _side() -> "torch.cuda.Stream":
    global _side_stream
    if _side_stream is None:
        _side_stream = torch.cuda.Stream()
    return _side_stream


def _side_dw_enabled() -> bool:
    """Opt-in (CI_SIDE_DW=1): compute dW_ih/db on a second HIP stream so
    they overlap the NEXT layer's sequential backward loop (which leaves
    ~40% of the chip idle). Only parameters with no other graph consumers
    (w_ih, b_ih, b_hh) are accumulated manually; dW_hh must return through
    autograd (the weight-drop mask backward consumes it). Anything that
    reads .grad after backward must call sync_dw_stream() first — the
    trainer does."""
    return os.environ.get("CI_SIDE_DW", "0") == "1"


def sync_dw_stream() -> None:
    """Order the side-stream weight-grad GEMMs before the current stream.
    No-op unless CI_SIDE_DW work was launched."""
    if _side_stream is not None and torch.cuda.is_available():
        torch.cuda.current_stream().wait_stream(_side_stream)


def _accum_grad(p: Tensor, g: Tensor) -> None:
    if p.grad is None:
        p.grad = g.detach().to(p.dtype)
    else:
        p.grad.add_(g.to(p.dtype))


def _fp8_weights(w_hh: Tensor):
    """Per-row e4m3 quantization of the recurrent weight (serving weights
    are static). CI_SERVE_FP8W=1 halves the weight stream that bounds
    small-batch serve latency. The cache lives ON the weight tensor
    (instance attribute) so its lifetime is the tensor's own — an id()
    keyed dict could hand back a stale quantization after the id is
    recycled post-GC (round-1 advisor finding)."""
    hit = getattr(w_hh, "_ci_fp8", None)
    if hit is not None and hit[0] == w_hh._version:
        return hit[1], hit[2]
    scale = w_hh.detach().abs().amax(dim=1, keepdim=True).float()         .clamp_min(1e-12) / 448.0
    q = (w_hh.detach().float() / scale).clamp(-448.0, 448.0)         .to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    out = (w_hh._version, q, scale.squeeze(1).contiguous())
    w_hh._ci_fp8 = out
    return out[1], out[2]


def _lstm_fp8_mode() -> str:
    """'' (off) | 'xp' (input projection only) | '1'/'all' (xp + recurrent).
    See _lstm_fp8_enabled for measurements."""
    return os.environ.get("CI_LSTM_FP8", "0")


def _lstm_fp8_enabled() -> bool:
    """CI_LSTM_FP8=1: run the training-path LSTM GEMMs in OCP e4m3 —
    the input projection via _scaled_mm (measured 8.8 -> 5.2 ms at the
    deployed layer shape) and the per-timestep recurrent GEMM with an
    e4m3 weight + the e4m3 hidden state the cell kernel emits for free
    (|h| < 1 so the h scale is a constant 1/448; 35 -> 28 us/call,
    scripts/lstm_fp8_probe.py). Backward stays bf16 from the bf16 saves.
    Off by default until the convergence gate in BENCH_HISTORY passes."""
    return _lstm_fp8_mode() in ("1", "all")


def _q8(lib, t: Tensor):
    """Per-tensor e4m3 quantize via the one-pass kernel; returns (q, scale)."""
    scale = (t.detach().abs().amax().float() / 448.0).clamp_min(1e-12)
    q = torch.empty(t.shape, dtype=torch.float8_e4m3fn, device=t.device)
    lib.quantize_e4m3(t.detach().contiguous(), q, scale)
    return q, scale


def _kmajor_dw(T: int, B: int, In: int, H: int, dt) -> bool:
    """Weight gradients through lstm_weight_grads (kmajor_pack.hip)?

    torch.mm(dg.t(), x) gives the library a GEMM with BOTH operands strided
    along K = T*B; with [x ; h_prev] packed K-major it runs one plain NN GEMM
    per layer instead (measured at T*B = 262144, profiles/BENCH_HISTORY.md:
    34.9 -> 27.7 ms at In = H = 2400 including the pack). The stacked GEMM's
    (In+H, 4H) output must still give every CU a 256x256 tile: below that
    the library's default choice for the new shape loses to the three tuned
    GEMMs (In=2400, H=800: 156 tiles, 8.8 vs 7.3 ms), which then stay.
    CI_LSTM_DW=legacy restores the three-GEMM form everywhere (A/B runs)."""
    if os.environ.get("CI_LSTM_DW", "") == "legacy":
        return False
    if dt not in (torch.bfloat16, torch.float32):
        return False
    if T * B < _KMAJOR_MIN_K:
        return True
    return (In + H) * 4 * H >= 256 * 256 * _n_cus()


# below this reduction length neither form is GEMM-bound (a few launches
# either way), so the tile rule has nothing to decide: small shapes take the
# same native path as the large layers
_KMAJOR_MIN_K = 4096
_cus = None


def _n_cus() -> int:
    global _cus
    if _cus is None:
        _cus = torch.cuda.get_device_properties(
            torch.cuda.current_device()).multi_processor_count
    return _cus


def _cpu_lstm_loop(x: Tensor, h0: Tensor, c0: Tensor, w_ih: Tensor, w_hh: Tensor,
                   b_ih: Tensor, b_hh: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """Pure-PyTorch reference (autograd-capable). x: (B,T,In)."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    xp = torch.addmm((b_ih + b_hh), x.reshape(B * T, -1), w_ih.t()).view(B, T, 4 * H)
    h, c = h0, c0
    outs = []
    for t in range(T):
        gates = xp[:, t] + h @ w_hh.t()
        i, f, g, o = gates.chunk(4, dim=1)
        i, f, g, o = i.sigmoid(), f.sigmoid(), g.tanh(), o.sigmoid()
        c = f * c + i * g
        h = o * torch.tanh(c)
        outs.append(h)
    return torch.stack(outs, dim=1), h, c


class _FusedLSTMFunction(torch.autograd.Function):
    """GPU path: HIP cell kernels over time-major saves, explicit backward."""

    @staticmethod
    def forward(ctx, x, h0, c0, w_ih, w_hh, b_ih, b_hh):
        lib = ext.require()
        B, T, In = x.shape
        H = w_hh.shape[1]
        dt = x.dtype
        # time-major input; free when x is already a (T,B,·) transpose view
        x_tm = x.transpose(0, 1).contiguous()
        bias = (b_ih + b_hh).to(torch.float32)
        # the drivers read h0/c0 as dense (B,H) rows: a strided view (e.g. a
        # column slice of a wider state tensor) is packed once, here
        h0 = h0.contiguous()
        c32 = c0.to(torch.float32).contiguous()
        shapes_ok = (dt == torch.bfloat16 and B > 8 and B % 16 == 0
                     and (T * B) % 16 == 0 and In % 16 == 0 and H % 16 == 0)
        fp8 = _lstm_fp8_enabled() and shapes_ok
        fp8_xp = fp8 or (_lstm_fp8_mode() == "xp" and shapes_ok)
        if fp8_xp:
            x2 = x_tm.view(T * B, In)
            x8, sx = _q8(lib, x2)
            wih8, swi = _q8(lib, w_ih)
            xp = torch._scaled_mm(x8, wih8.t(), scale_a=sx, scale_b=swi,
                                  out_dtype=dt).view(T, B, 4 * H)
        else:
            xp = torch.mm(x_tm.view(T * B, In), w_ih.t()).view(T, B, 4 * H)
        hs = torch.empty(T, B, H, dtype=dt, device=x.device)
        cs = torch.empty(T, B, H, dtype=torch.float32, device=x.device)
        gates = torch.empty(T, B, 4 * H, dtype=dt, device=x.device)
        # default "lib": hipBLASLt recurrent GEMM + fused pointwise cell
        # kernel — measured faster than the fully fused MFMA cell kernel
        # (471 vs 492 ms/step at the deployed shape, profiles/BENCH_HISTORY.md);
        # CI_LSTM_MODE=fused selects the hand-written fused path.
        mode = os.environ.get("CI_LSTM_MODE", "lib")
        if dt == torch.bfloat16 and B <= 8 and mode != "lib-only":
            # serve/decode regime: weight-streaming-bound GEMV — the fused
            # GEMV+cell kernel replaces hipBLASLt GEMV + pointwise launch
            if os.environ.get("CI_SERVE_FP8W", "0") == "1"                     and not torch.is_grad_enabled():
                w8, wscale = _fp8_weights(w_hh)
                lib.lstm_seq_forward_gemv_fp8(xp, bias, h0, c32, w8,
                                              wscale, hs, cs, gates)
            elif os.environ.get("CI_SERVE_PERSISTENT", "0") == "1" \
                    and not getattr(_FusedLSTMFunction, "_pers_failed", False):
                # whole-sequence persistent grid: one launch per layer,
                # software grid barrier between timesteps. The kernel
                # bails (fail flag) instead of hanging if the grid is
                # not co-resident; fall back per-step then.
                ws = torch.zeros(4, dtype=torch.int32, device=x.device)
                nb = lib.lstm_seq_forward_gemv_persistent(
                    xp, bias, h0, c32, w_hh, hs, cs, gates, ws)
                if nb == 0 or int(ws[2].item()) != 0:
                    import warnings
                    warnings.warn("persistent GEMV unavailable "
                                  f"(nb={nb}); per-step fallback (sticky)")
                    _FusedLSTMFunction._pers_failed = True  # stop re-bailing
                    lib.lstm_seq_forward_gemv(xp, bias, h0, c32,
                                              w_hh, hs, cs, gates)
            else:
                lib.lstm_seq_forward_gemv(xp, bias, h0, c32,
                                          w_hh, hs, cs, gates)
        elif dt == torch.bfloat16 and H % 8 == 0 and (
                mode == "fused"
                or (mode == "auto" and H >= 2048 and B >= 128)):
            # "auto": fused MFMA cell only where its grid fills the chip
            # (H=2400 layers -> 600 blocks); small layers stay on lib
            lib.lstm_seq_forward_fused(xp, bias, h0, c32, w_hh,
                                       hs, cs, gates)
        elif fp8 and mode == "lib":
            whh8, swh = _q8(lib, w_hh)
            lib.lstm_seq_forward_lib_fp8(xp, bias, h0, c32, whh8, swh,
                                         hs, cs, gates)
        else:
            lib.lstm_seq_forward_lib(xp, bias, h0, c32, w_hh,
                                     hs, cs, gates)
        ctx.save_for_backward(x_tm, h0, c0, w_ih, w_hh, gates, hs, cs)
        ctx.direct_params = (w_ih, b_ih, b_hh)  # no other graph consumers
        hT = hs[-1].clone()
        cT = cs[-1].to(dt)
        out = hs.transpose(0, 1)  # (B,T,H) view of time-major storage
        return out, hT, cT

    @staticmethod
    def backward(ctx, dhs, dhT, dcT):
        lib = ext.require()
        x_tm, h0, c0, w_ih, w_hh, gates, hs, cs = ctx.saved_tensors
        T, B, In = x_tm.shape
        H = w_hh.shape[1]
        dt = x_tm.dtype
        dhs_tm = dhs.transpose(0, 1).contiguous()
        dgates = torch.empty(T, B, 4 * H, dtype=dt, device=x_tm.device)
        dh0 = torch.empty(B, H, dtype=torch.float32, device=x_tm.device)
        # carried state is detached in training: then the step-0 dh GEMM
        # (fp32, from unrounded dgates) is skipped and no dh0 is returned
        need_dh0 = ctx.needs_input_grad[1]
        dc0 = torch.empty(B, H, dtype=torch.float32, device=x_tm.device)
        lib.lstm_seq_backward(dhs_tm, dhT.contiguous(),
                              dcT.to(torch.float32).contiguous(),
                              gates, hs, cs,
                              c0.to(torch.float32).contiguous(), w_hh,
                              dgates, dh0, dc0, need_dh0)
        dh0_out = dh0.to(dt) if need_dh0 else None
        dg2 = dgates.view(T * B, 4 * H)
        dx_tm = torch.mm(dg2, w_ih).view(T, B, In)
        need_ih, need_hh = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        side = _side_dw_enabled() and need_ih
        if side or not _kmajor_dw(T, B, In, H, dt):
            # dW_hh = sum_t h_{t-1}^T dgates_t — time-major slices stay
            # contiguous, so no (T,B,H) cat materializes:
            dw_hh = torch.mm(dgates[0].t(), h0.to(dt))
            if T > 1:
                dw_hh += torch.mm(dgates[1:].reshape((T - 1) * B, 4 * H).t(),
                                  hs[:-1].reshape((T - 1) * B, H))
            dw_ih = None
        else:
            # [x ; h_prev] written K-major once, then ONE row-major GEMM per
            # layer instead of three with both operands strided along K
            dw_ih, dw_hh = lib.lstm_weight_grads(dgates, x_tm, hs, h0.to(dt),
                                                 need_ih, need_hh)
        if side:
            # overlap dW_ih/db with the next layer's sequential loop
            # (never for a frozen layer: its .grad must stay None)
            pw, pbi, pbh = ctx.direct_params
            s_ = _side()
            s_.wait_stream(torch.cuda.current_stream())
            dg2.record_stream(s_)
            x_tm.record_stream(s_)
            with torch.cuda.stream(s_):
                dw_ih_s = torch.mm(dg2.t(), x_tm.view(T * B, In))
                db_s = dg2.sum(dim=0)
                _accum_grad(pw, dw_ih_s)
                _accum_grad(pbi, db_s)
                # clone: assigning the SAME tensor as both .grads would alias
                # them and double-count on later accumulation micro-steps
                _accum_grad(pbh, db_s.clone())
            return (dx_tm.transpose(0, 1), dh0_out, dc0.to(dt),
                    None, dw_hh.to(w_hh.dtype), None, None)
        if dw_ih is None and need_ih:
            dw_ih = torch.mm(dg2.t(), x_tm.view(T * B, In))
        db = dg2.sum(dim=0).to(dt)
        return (dx_tm.transpose(0, 1), dh0_out, dc0.to(dt),
                dw_ih.to(w_ih.dtype) if dw_ih is not None else None,
                dw_hh.to(w_hh.dtype) if dw_hh is not None else None,
                db, db.clone())


def lstm_forward(x: Tensor, h0: Tensor, c0: Tensor, w_ih: Tensor, w_hh: Tensor,
                 b_ih: Tensor, b_hh: Tensor):
    """Run one LSTM layer over (B,T,In). Returns (out (B,T,H), (hT, cT))."""
    if x.is_cuda:
        hs, hT, cT = _FusedLSTMFunction.apply(x, h0, c0, w_ih, w_hh, b_ih, b_hh)
        return hs, (hT, cT)
    out, h, c = _cpu_lstm_loop(x, h0, c0, w_ih, w_hh, b_ih, b_hh)
    return out, (h, c)
