"""CPU checks of the fp64 CE references in ce_ref.py. They keep the
reference the GPU tests lean on independent of project code (validated
against torch's own logsumexp / cross_entropy / autograd) and show that
every derived bound is at least 2x below what a realistic kernel error
would cause, for every case the GPU tests run.

Input scales of the end-to-end cases (ce_ref.SCALES): h 0.5, w 0.2, b 0.1,
and for the fp8 recompute path also h 2.0, w 0.4. At both, every wrong
variant clears 2x the bound on at least one output on every path, the fp8
ones included, so no scale had to be changed for the guard to hold."""
import pytest
import torch

import ce_ref as C

D = torch.float64


# ---- the references themselves ---------------------------------------------

@pytest.mark.parametrize("has_bias", [False, True])
def test_ce_exact_matches_torch_cross_entropy_and_autograd(has_bias):
    torch.manual_seed(3)
    N, H, V = 9, 5, 13
    h = torch.randn(N, H, dtype=D, requires_grad=True)
    w = torch.randn(V, H, dtype=D, requires_grad=True)
    b = torch.randn(V, dtype=D, requires_grad=True) if has_bias else None
    t = torch.randint(0, V, (N,))
    loss = C.ce_exact(h, w, b, t)
    want = torch.nn.functional.cross_entropy(
        torch.nn.functional.linear(h, w, b), t)
    tol = dict(rtol=1e-12, atol=1e-14)
    assert torch.allclose(loss, want, **tol)
    (0.5 * loss).backward()
    got = C.ce_exact_grads(h.detach(), w.detach(),
                           None if b is None else b.detach(), t, dloss=0.5)
    assert torch.allclose(got["loss"], want, **tol)
    assert torch.allclose(got["dh"], h.grad, **tol)
    assert torch.allclose(got["dW"], w.grad, **tol)
    if has_bias:
        assert torch.allclose(got["db"], b.grad, **tol)
    else:
        assert got["db"] is None


def test_epilogue_exact_matches_torch():
    torch.manual_seed(4)
    x = torch.randn(4, 11, dtype=D) * 3
    b = torch.randn(11, dtype=D)
    t = torch.tensor([0, 10, 7, 8])
    ex = C.epilogue_exact(x, b, t, 0.25)
    z = x + b
    tol = dict(rtol=1e-12, atol=1e-14)
    assert torch.allclose(ex["lse"], torch.logsumexp(z, 1), **tol)
    assert torch.allclose(ex["tgt"], z[torch.arange(4), t], **tol)
    assert torch.allclose(ex["p"], torch.softmax(z, 1), **tol)
    onehot = torch.nn.functional.one_hot(t, 11).to(D)
    assert torch.allclose(ex["q"], (torch.softmax(z, 1) - onehot) * 0.25,
                          **tol)
    assert torch.allclose(ex["q8"], (torch.softmax(z, 1) - onehot) * 448,
                          **tol)
    # the tail_max_ignored variant is the exact lse unless a row's maximum
    # sits in the tail
    x[:, 8:] = x[:, 8:].clamp_max(float(x[:, :8].min()))
    ok = C.epilogue_exact(x, b * 0, t, 0.25, wrong="tail_max_ignored")
    assert torch.allclose(ok["lse"], torch.logsumexp(x, 1), **tol)


def test_half_ulp_and_e4m3_step_match_the_formats():
    """The rounding-error helpers against torch's own casts: the worst
    rounding error over a dense sweep reaches the bound and never passes
    it."""
    x = torch.logspace(-4, 2.6, 20001, dtype=D)
    for dt in (torch.bfloat16, torch.float32):
        err = (x.to(dt).double() - x).abs()
        hu = C.half_ulp(x, dt)
        assert (err <= hu).all()
        assert (err / hu).max() > 0.95
    err = (x.float().to(C.F8).double() - x).abs()
    hs = C.e4m3_half_step(x)
    assert (err <= hs).all()
    assert (err / hs).max() > 0.95
    assert float(C.e4m3_half_step(torch.tensor([1e-5], dtype=D))) == 2.0 ** -10


def test_models_sit_where_their_formats_put_them():
    """fp32 model within 1e-6 of ce_exact; bf16 model within the bf16 bound
    (K * E + floor with E from the model is trivially met, so the check is
    against the format: logits rounded to bf16, half-ulp 2^-9 relative at
    most 2^-8, move loss and gradients by bf16-sized relative amounts)."""
    for path, lo, hi in (("fp32", 0.0, 1e-6), ("bf16", 1e-6, 2.0 ** -7)):
        for c in C.e2e_cases():
            if c["path"] != path:
                continue
            case = C.e2e_case(c)
            for k in case["keys"]:
                scale = float(case["exact"][k].abs().max())
                rel = case["E"][k] / scale
                assert rel <= hi, (C.e2e_case_id(c), k, rel)
            assert case["E"]["dW"] / float(
                case["exact"]["dW"].abs().max()) >= lo


# ---- the bounds can see realistic errors -----------------------------------

@pytest.mark.parametrize("case", C.epilogue_cases(), ids=C.epilogue_case_id)
def test_epilogue_bounds_catch_wrong_variants(case):
    dt, V, has_bias, kind, tset = case
    c = C.epilogue_case(case)
    outs = ("lse", "tgt", "q", "q8")
    # the exact values sit inside their own bound
    for k in outs:
        assert C.worst_ratio(c["exact"][k], c["exact"][k],
                             c["allowed"][k]) == 0.0
    for wrong in C.WRONG_EPILOGUE:
        if not C.wrong_applies(wrong, has_bias, V, c["vec"]):
            continue
        bad = C.epilogue_exact(c["logits"], c["bias"], c["targets"],
                               c["scale"], wrong=wrong, vec=c["vec"])
        moved = max(C.worst_ratio(bad[k], c["exact"][k], c["allowed"][k])
                    for k in outs)
        assert moved >= 2.0, (wrong, moved)


@pytest.mark.parametrize("c", C.e2e_cases(), ids=C.e2e_case_id)
def test_e2e_bounds_catch_wrong_variants(c):
    case = C.e2e_case(c)
    fp8 = c["path"].startswith("fp8")
    for k in case["keys"]:       # the model itself is inside K * E + floor
        assert C.worst_ratio(case["model"][k], case["exact"][k],
                             case["allowed"][k] + 0 * case["exact"][k]) <= 1
    for wrong in C.WRONG_E2E:
        if wrong.startswith("bias") and not c["bias"]:
            continue
        if wrong == "store_missing" and not fp8:
            continue
        bad = C.ce_exact_grads(case["h"], case["w"], case["b"], case["t"],
                               c["dloss"], wrong=wrong, fp8_dh=fp8)
        moved = max(C.worst_ratio(bad[k], case["exact"][k],
                                  case["allowed"][k] + 0 * case["exact"][k])
                    for k in case["keys"])
        assert moved >= 2.0, (wrong, moved)


def test_db_sum_bound_sees_a_softmax_that_does_not_sum_to_one():
    """db.sum() is 0 exactly. The model's own value must sit inside the
    derived bound, and an lse that is off by 0.1 on every row (p scaled by
    e^0.1: the rows sum to 1.105) must miss it by more than 2x."""
    for c in C.e2e_cases():
        if c["path"] != "fp8_recompute" or not c["bias"]:
            continue
        case = C.e2e_case(c)
        allowed = case["db_sum_allowed"]
        assert abs(float(case["model"]["db"].sum())) <= allowed
        off = c["dloss"] * (torch.exp(torch.tensor(0.1, dtype=D)) - 1)
        assert float(off) > 2 * allowed, (float(off), allowed)


# ---- quantize_e4m3 ---------------------------------------------------------

def test_quantize_tie_inputs_split_division_from_reciprocal():
    """The inputs the GPU test uses: for each, x / 7 is an exact e4m3 tie
    and x * (1/7) gives the other code, so a kernel that multiplies by the
    reciprocal anywhere cannot pass by luck."""
    ties = C.tie_inputs()
    assert ties.numel() >= 8          # a full bf16 vector of them
    a = C.quantize_exact(ties, C.TIE_SCALE).view(torch.uint8)
    b = C.quantize_by_reciprocal(ties, C.TIE_SCALE).view(torch.uint8)
    assert (a != b).all()
    assert (ties.to(torch.bfloat16).float() == ties).all()
    for dt in (torch.bfloat16, torch.float32):
        for n in C.QUANT_SIZES:
            x = C.quantize_input(n, dt)
            assert x.shape == (n,)
            a = C.quantize_exact(x, C.TIE_SCALE).view(torch.uint8)
            b = C.quantize_by_reciprocal(x, C.TIE_SCALE).view(torch.uint8)
            assert (a != b).any(), (dt, n)
            vec = C.vec_of(dt)
            if n % vec and n > vec:   # ties both in the tail and before it
                tail = n - n % vec
                assert (a[tail:] != b[tail:]).any(), (dt, n)
                assert (a[:tail] != b[:tail]).any(), (dt, n)


def test_quantize_exact_saturates_and_keeps_nan():
    x = torch.tensor([4000.0, -4000.0, float("nan"), 0.0, 7 * 2.0 ** -10])
    q = C.quantize_exact(x, C.TIE_SCALE).view(torch.uint8)
    assert q[0] == 0x7e and q[1] == 0xfe          # +-448
    assert q[2] & 0x7f == 0x7f                    # NaN code
    assert q[3] == 0 and q[4] == 0                # zero; tie flushes to even
