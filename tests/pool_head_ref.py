"""fp64 reference and first-order forward-error bound for the pooling head
(BatchNorm1d -> Dropout -> Linear [-> ReLU -> ...]) in eval mode; shared by
test_gpu_pool_stream.py and test_gpu_classifier_predict.py, which derive it
in their docstrings."""
import torch

U = 2.0 ** -24                      # fp32 unit roundoff


def gamma(k):
    return k * U / (1 - k * U)


def bn_affine(bn):
    """Eval-mode BatchNorm as x * s + t, in fp64."""
    s = bn.weight.double() / (bn.running_var.double() + bn.eps).sqrt()
    return s, bn.bias.double() - bn.running_mean.double() * s


@torch.no_grad()
def head_bounds(head, f, feat_err=None, roundings=4, terms=None):
    """Exact fp64 logits of ``head`` on fp64 features ``f`` (B, n_in), and a
    bound E (B, C) on the error of an fp32 evaluation of them.

    Per layer, with x its exact input and Ex the error already in it:
      A_j = sum_k |W_jk| (|x_k s_k| + |t_k|) + |b_j|
      E_j = gamma(K + roundings) * A_j + sum_k |W_jk s_k| Ex_k
    K - 1 additions in any order plus ``roundings`` more roundings per term;
    relu is 1-Lipschitz. ``feat_err`` is Ex of the first layer. ``terms``
    replaces K + roundings by a fixed count (1: the only rounding is that of
    each weight and bias, as when fp32-folded weights are applied in fp64)."""
    mods = list(head.layers)
    pairs = [(mods[i], mods[i + 2]) for i in range(0, len(mods), 4)]
    x = f
    E = torch.zeros_like(f) if feat_err is None else feat_err
    for i, (bn, lin) in enumerate(pairs):
        s, t = bn_affine(bn)
        W, b = lin.weight.double(), lin.bias.double()
        z = (x * s + t) @ W.t() + b
        A = ((x * s).abs() + t.abs()) @ W.abs().t() + b.abs()
        k = W.size(1) + roundings if terms is None else terms
        E = gamma(k) * A + E @ (W * s).abs().t()
        x = torch.relu(z) if i != len(pairs) - 1 else z
    return z, E
