"""LSTM weight gradients through lstm_weight_grads (kmajor_pack.hip): the
K-major pack of [x ; h_prev] plus one stacked GEMM, against fp64.

Reference: dW_ih = dg^T x and dW_hh = dg^T h_prev in fp64 from the same,
already rounded inputs; h_prev[0] = h0 (non-zero), h_prev[t] = hs[t-1].

Bound per element (from the formats, not from the kernel):
  * fp32 accumulation of a K = T*B term dot product: K 2^-24 sum|a b|
    (the standard bound; it covers the final fp32 rounding);
  * bf16 only: half a bf16 ulp AT the reference value for the one rounding
    of the stored result (the output transposes move bits).
The CPU tests show that a plain fp32-accumulate / bf16-round model of the
GEMM meets the bound and that three wrong computations (h_prev not shifted
by one step, h0 dropped, ih/hh blocks swapped) miss it by more than 2x.

End to end (lstm_forward, CI_LSTM_DW unset vs legacy) the backward kernels
are the same, so dx, dh0, dc0 and db must be bit-equal. The weight
gradients of both paths are held against the fp64 product of the dgates
the backward actually produced (captured at the lstm_weight_grads call):
the new path within the bound above; the legacy path, which rounds dW_hh's
two partial products to bf16 before adding them, within the bound plus
half an ulp of each partial. Two correctly rounded results of sums that
differ in the last fp32 bits can sit on adjacent bf16 values, a whole ulp
apart, so comparing the two paths with each other under a half-ulp bound
would fail correct code; each is compared with the exact value instead.

Measured on MI355X, max |error| / bound over the cases: direct calls bf16
0.999 (the half-ulp term is nearly all of the bound, and some element
always rounds from close to a tie), fp32 0.174; end to end new path bf16
0.997, fp32 0.080; legacy path bf16 0.997, fp32 0.052.
"""
import pytest
import torch

from ce_ref import BF16, F32, half_ulp, worst_ratio

SHAPES = [(1, 16, 16, 16), (3, 16, 24, 40), (4, 32, 48, 16)]  # (T, B, In, H)
DTYPES = [BF16, F32]
EPS32 = 2.0 ** -24

_cache = {}


def _case(shape, dtype):
    """Inputs rounded to dtype, fp64 references and bounds; read-only."""
    key = (shape, dtype)
    if key in _cache:
        return _cache[key]
    T, B, In, H = shape
    g = torch.Generator().manual_seed(sum(shape) + (dtype == F32))
    dg = (0.3 * torch.randn(T, B, 4 * H, generator=g)).to(dtype)
    x = torch.randn(T, B, In, generator=g).to(dtype)
    hs = torch.tanh(torch.randn(T, B, H, generator=g)).to(dtype)
    h0 = (0.5 * torch.randn(B, H, generator=g)).to(dtype)
    c = dict(dg=dg, x=x, hs=hs, h0=h0, **_reference(dg, x, hs, h0, dtype))
    _cache[key] = c
    return c


def _hprev(hs, h0, wrong=None):
    if wrong == "not_shifted":
        return hs
    if wrong == "h0_dropped":
        h0 = torch.zeros_like(h0)
    return torch.cat([h0[None], hs[:-1]], dim=0)


def _reference(dg, x, hs, h0, dtype, wrong=None):
    """fp64 (dw_ih, dw_hh) and the allowed error of each."""
    T, B, G = dg.shape
    K = T * B
    dg2 = dg.double().reshape(K, G)
    x2 = x.double().reshape(K, -1)
    hp2 = _hprev(hs, h0, wrong).double().reshape(K, -1)
    if wrong == "blocks_swapped":
        # the stacked operand built as [h_prev ; x] but split as [x ; h_prev]
        In = x2.shape[1]
        st = dg2.t() @ torch.cat([hp2, x2], dim=1)
        return dict(dw_ih=st[:, :In], dw_hh=st[:, In:])
    out = {}
    for name, a in (("dw_ih", x2), ("dw_hh", hp2)):
        ref = dg2.t() @ a
        allowed = K * EPS32 * (dg2.abs().t() @ a.abs())
        if dtype == BF16:
            allowed = allowed + half_ulp(ref, BF16)
        out[name] = ref
        out[name + "_allowed"] = allowed
    return out


def _ids(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return "bf16" if v == BF16 else "fp32"


both = pytest.mark.parametrize("shape", SHAPES, ids=_ids)
dts = pytest.mark.parametrize("dtype", DTYPES, ids=_ids)


# ---- CPU: the bound itself ---------------------------------------------------

@both
@dts
def test_bound_holds_for_fp32_accumulate_model(shape, dtype):
    c = _case(shape, dtype)
    T, B, _, _ = shape
    dg2 = c["dg"].float().reshape(T * B, -1)
    for name, a in (("dw_ih", c["x"]), ("dw_hh", _hprev(c["hs"], c["h0"]))):
        model = (dg2.t() @ a.float().reshape(T * B, -1)).to(dtype)
        r = worst_ratio(model, c[name], c[name + "_allowed"])
        assert r <= 1.0, (name, r)


@both
@dts
@pytest.mark.parametrize("wrong", ["not_shifted", "h0_dropped",
                                   "blocks_swapped"])
def test_bound_rejects_wrong_reference(shape, dtype, wrong):
    c = _case(shape, dtype)
    bad = _reference(c["dg"], c["x"], c["hs"], c["h0"], dtype, wrong=wrong)
    # x does not enter the first two: only dw_hh can tell
    names = ("dw_ih", "dw_hh") if wrong == "blocks_swapped" else ("dw_hh",)
    for name in names:
        assert bad[name].shape == c[name].shape
        r = worst_ratio(bad[name], c[name], c[name + "_allowed"])
        assert r > 2.0, (name, r)


# ---- GPU: the native op ------------------------------------------------------

@pytest.mark.gpu
@both
@dts
def test_lstm_weight_grads_vs_fp64(shape, dtype):
    from code_intelligence_amd.ops import extension as ext
    lib = ext.require()
    c = _case(shape, dtype)
    args = [c[k].cuda() for k in ("dg", "x", "hs", "h0")]
    dw_ih, dw_hh = lib.lstm_weight_grads(*args)
    T, B, In, H = shape
    assert dw_ih.shape == (4 * H, In) and dw_hh.shape == (4 * H, H)
    assert dw_ih.is_contiguous() and dw_hh.is_contiguous()
    assert dw_ih.dtype == dtype and dw_hh.dtype == dtype
    for name, got in (("dw_ih", dw_ih), ("dw_hh", dw_hh)):
        r = worst_ratio(got.cpu(), c[name], c[name + "_allowed"])
        print(f"lstm_weight_grads {_ids(shape)} {_ids(dtype)} {name}: "
              f"max err/bound = {r:.3f}")
        assert r <= 1.0, (name, r)
    # only one gradient wanted: the other is not computed, the wanted one
    # still meets the bound (its GEMM has another shape)
    only_hh = lib.lstm_weight_grads(*args, need_ih=False)
    assert only_hh[0] is None
    assert worst_ratio(only_hh[1].cpu(), c["dw_hh"],
                       c["dw_hh_allowed"]) <= 1.0
    only_ih = lib.lstm_weight_grads(*args, need_hh=False)
    assert only_ih[1] is None
    assert worst_ratio(only_ih[0].cpu(), c["dw_ih"],
                       c["dw_ih_allowed"]) <= 1.0
    assert lib.lstm_weight_grads(*args, need_ih=False,
                                 need_hh=False) == (None, None)


E2E = (16, 4, 32, 48)  # (B, T, In, H)


def _run_layer(dtype, monkeypatch, legacy, freeze_ih=False):
    """One lstm_forward + backward on the GPU. Returns the gradients and,
    on the new path, the tensors lstm_weight_grads was called with."""
    from code_intelligence_amd.ops import extension as ext
    from code_intelligence_amd.ops.lstm import lstm_forward
    lib = ext.require()
    if legacy:
        monkeypatch.setenv("CI_LSTM_DW", "legacy")
    else:
        monkeypatch.delenv("CI_LSTM_DW", raising=False)
    monkeypatch.delenv("CI_SIDE_DW", raising=False)
    seen = []
    real = lib.lstm_weight_grads

    def spy(*a, **k):
        seen.append([t.detach().clone() if isinstance(t, torch.Tensor) else t
                     for t in a])
        return real(*a, **k)

    monkeypatch.setattr(lib, "lstm_weight_grads", spy)
    B, T, In, H = E2E
    g = torch.Generator().manual_seed(5)

    def leaf(*shape, scale=1.0, grad=True):
        return (scale * torch.randn(*shape, generator=g)).to(dtype).cuda() \
            .requires_grad_(grad)

    x = leaf(B, T, In)
    h0, c0 = leaf(B, H, scale=0.5), leaf(B, H, scale=0.5)
    w_ih = leaf(4 * H, In, scale=0.2, grad=not freeze_ih)
    w_hh = leaf(4 * H, H, scale=0.2)
    b_ih, b_hh = leaf(4 * H, scale=0.1), leaf(4 * H, scale=0.1)
    wo = (torch.randn(B, T, H, generator=g)).to(dtype).cuda()
    out, (hT, cT) = lstm_forward(x, h0, c0, w_ih, w_hh, b_ih, b_hh)
    ((out * wo).sum() + hT.sum() + 0.5 * cT.sum()).backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(lib, "lstm_weight_grads", real)
    grads = dict(dx=x.grad, dh0=h0.grad, dc0=c0.grad, dw_ih=w_ih.grad,
                 dw_hh=w_hh.grad, db_ih=b_ih.grad, db_hh=b_hh.grad)
    return grads, seen


@pytest.mark.gpu
@dts
def test_lstm_layer_new_vs_legacy(dtype, monkeypatch):
    new, seen = _run_layer(dtype, monkeypatch, legacy=False)
    old, seen_old = _run_layer(dtype, monkeypatch, legacy=True)
    assert len(seen) == 1 and not seen_old  # each ran the path it names
    for k in ("dx", "dh0", "dc0", "db_ih", "db_hh"):
        assert torch.equal(new[k], old[k]), k
    dg, x_tm, hs, h0 = [t.cpu() for t in seen[0][:4]]
    ref = _reference(dg, x_tm, hs, h0, dtype)
    T, B = dg.shape[:2]
    for name in ("dw_ih", "dw_hh"):
        r = worst_ratio(new[name].cpu(), ref[name], ref[name + "_allowed"])
        print(f"lstm layer {_ids(dtype)} new {name}: err/bound = {r:.3f}")
        assert r <= 1.0, (name, r)
        allowed = ref[name + "_allowed"]
        if name == "dw_hh" and dtype == BF16:
            # legacy: bf16(bf16(dg[0]^T h0) + bf16(dg[1:]^T hs[:-1]))
            p0 = dg[0].double().t() @ h0.double()
            allowed = allowed + half_ulp(p0, BF16) \
                + half_ulp(ref[name] - p0, BF16)
        r = worst_ratio(old[name].cpu(), ref[name], allowed)
        print(f"lstm layer {_ids(dtype)} legacy {name}: err/bound = {r:.3f}")
        assert r <= 1.0, (name, r)


@pytest.mark.gpu
@dts
def test_lstm_layer_frozen_w_ih(dtype, monkeypatch):
    got, seen = _run_layer(dtype, monkeypatch, legacy=False, freeze_ih=True)
    assert got["dw_ih"] is None
    assert len(seen) == 1
    dg, x_tm, hs, h0, need_ih, need_hh = seen[0]
    assert (need_ih, need_hh) == (False, True)
    ref = _reference(dg.cpu(), x_tm.cpu(), hs.cpu(), h0.cpu(), dtype)
    assert worst_ratio(got["dw_hh"].cpu(), ref["dw_hh"],
                       ref["dw_hh_allowed"]) <= 1.0
    assert got["dx"] is not None and got["db_ih"] is not None
