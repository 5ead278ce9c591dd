"""CPU checks of the fp64 LSTM references in lstm_ref.py. They keep the
reference the GPU kernel tests lean on independent of project code: it is
validated against torch.nn.LSTM, not against the op under test."""
import pytest
import torch

import lstm_ref as R


@pytest.mark.parametrize("shape", [(3, 1, 4, 5), (4, 3, 6, 7)])
def test_ref_exact_matches_nn_lstm_fp64(shape):
    """Outputs, final state and all seven gradients with non-zero carried
    state and a loss that depends on out, hT and cT."""
    B, T, In, H = shape
    torch.manual_seed(5)
    D = torch.float64
    lstm = torch.nn.LSTM(In, H, batch_first=True).to(D)
    x = torch.randn(B, T, In, dtype=D, requires_grad=True)
    h0 = (0.5 * torch.randn(B, H, dtype=D)).requires_grad_(True)
    c0 = (0.5 * torch.randn(B, H, dtype=D)).requires_grad_(True)
    g_out = torch.randn(B, T, H, dtype=D)
    g_hT = torch.randn(B, H, dtype=D)
    g_cT = torch.randn(B, H, dtype=D)

    out, (hT, cT) = lstm(x, (h0[None], c0[None]))
    torch.autograd.backward([out, hT[0], cT[0]], [g_out, g_hT, g_cT])
    params = [lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0,
              lstm.bias_hh_l0]
    want = [t.grad.clone() for t in [x, h0, c0] + params]
    for t in [x, h0, c0] + params:
        t.grad = None

    hs, cs, gates = R.ref_exact(x, h0, c0, *params)
    torch.autograd.backward([hs.transpose(0, 1), hs[-1], cs[-1]],
                            [g_out, g_hT, g_cT])
    got = [t.grad for t in [x, h0, c0] + params]

    tol = dict(rtol=1e-10, atol=1e-13)
    assert torch.allclose(hs.transpose(0, 1), out, **tol)
    assert torch.allclose(hs[-1], hT[0], **tol)
    assert torch.allclose(cs[-1], cT[0], **tol)
    assert gates.shape == (T, B, 4 * H)
    for name, g, w in zip(("x", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh"),
                          got, want):
        assert torch.allclose(g, w, **tol), (name, (g - w).abs().max())


def test_ref_model_without_rounding_error_is_ref_exact():
    """At fp32 storage the model's roundings are ~1e-7: it must sit on top
    of ref_exact, and the bf16 model must differ by bf16-sized amounts."""
    c = R.forward_case("lib_fp32", 5, 6, 3)
    assert max(c["E"].values()) < 5e-6, c["E"]
    c = R.forward_case("lib_bf16", 5, 20, 3)
    assert 1e-4 < c["E"]["hs"] < 0.02, c["E"]


def test_cell_backward_exact_matches_autograd():
    """dgates (the gradient of the pre-activations), dh0 and dc0 of the
    closed form vs autograd through an independently written cell."""
    torch.manual_seed(6)
    B, H = 3, 5
    D = torch.float64
    pre = torch.randn(B, 4 * H, dtype=D).requires_grad_(True)  # xp + bias
    h0 = torch.randn(B, H, dtype=D).requires_grad_(True)
    c0 = torch.randn(B, H, dtype=D).requires_grad_(True)
    w = (0.3 * torch.randn(4 * H, H, dtype=D))
    z = pre + h0 @ w.t()           # d loss / d pre == d loss / d z == dgates
    i, f, g, o = z.split(H, dim=1)
    i, f, g, o = i.sigmoid(), f.sigmoid(), g.tanh(), o.sigmoid()
    c = f * c0 + i * g
    h = o * c.tanh()
    dh, dhT, dcT = (torch.randn(B, H, dtype=D) for _ in range(3))
    torch.autograd.backward([h, h, c], [dh, dhT, dcT])
    gates = torch.cat([i, f, g, o], dim=1).detach()
    dg, dh0, dc0 = R.cell_backward_exact(dh, dhT, dcT, gates, c0.detach(),
                                         c.detach(), w)
    tol = dict(rtol=1e-10, atol=1e-13)
    assert torch.allclose(dg, pre.grad, **tol)
    assert torch.allclose(dh0, h0.grad, **tol)
    assert torch.allclose(dc0, c0.grad, **tol)


@pytest.mark.parametrize("driver", R.DRIVERS)
def test_bounds_catch_permutation_errors(driver):
    """For every forward case of the GPU tests: swapping any two gates or
    shifting the hidden-unit index by one moves hs, cs and gates by more
    than the allowed error, so the derived bound can see such a bug."""
    for (d, B, H, T) in R.all_forward_cases():
        if d != driver:
            continue
        c = R.forward_case(d, B, H, T)
        for k in ("hs", "cs", "gates"):
            assert c["moved"][k] > 2 * c["allowed"][k], \
                (d, B, H, T, k, c["moved"][k], c["allowed"][k])
