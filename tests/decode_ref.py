"""fp64 references and error bounds shared by the decode-and-sample tests.

Everything here is computed from the already dtype-rounded inputs, in fp64,
in fastai's order: softmax, zero ``unk``, ``min_p`` mask (skipped when nothing
would survive), ``pow(1 / temperature)``, explicit ``cumsum``.
"""
import math

import torch

U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


def inputs(B, V, H, dtype, with_bias, seed, spikes=None):
    """Near-uniform next-word distribution (logit std ~0.1) so that almost
    every token's CDF interval is far wider than the fp32 error bounds;
    ``spikes`` {index: logit offset} go into the bias."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, H, generator=g)
    w = torch.randn(V, H, generator=g) * (0.1 / H ** 0.5)
    bias = None
    if with_bias:
        bias = 0.05 * torch.randn(V, generator=g)
        for i, off in (spikes or {}).items():
            bias[i] += off
        bias = bias.to(dtype)
    return h.to(dtype), w.to(dtype), bias


def logits_ref(h, w, bias):
    """(l64, E): exact logits of the rounded inputs and the per-element fp32
    bound gamma(H+2) * (sum_k |W_vk h_bk| + |bias_v|)."""
    h64, w64 = h.double(), w.double()
    l64 = h64 @ w64.t()
    A = h64.abs() @ w64.abs().t()
    if bias is not None:
        l64 = l64 + bias.double()
        A = A + bias.double().abs()
    return l64, gamma(h.size(1) + 2) * A


def fastai_weights(l64_row, unk, min_p, temperature):
    """One row. Returns (p64, kept mask, weights) in fastai's order."""
    p = torch.softmax(l64_row, dim=0)
    res = p.clone()
    if unk >= 0:
        res[unk] = 0.0
    if min_p is not None:
        if (res >= min_p).double().sum() == 0:
            pass            # fastai warns and samples unfiltered
        else:
            res[res < min_p] = 0.0
    kept = res > 0
    return p, kept, res.pow(1.0 / temperature)


def cdf(weights):
    """Normalised running sums F (F[-1] == 1), an explicit ascending cumsum."""
    F = torch.empty_like(weights)
    acc = 0.0
    for i, x in enumerate(weights.tolist()):
        acc += x
        F[i] = acc
    return F / acc


def cdf_tol(E_row, l64_row, kept, weights, V, temperature):
    """Bound on |S_t / S_V - F_t| for running sums S computed in fp32 from
    fp32 logits within E of l64 (derivation: test_gpu_decode.py)."""
    Ek = E_row[kept]
    mean_E = float((weights[kept] * Ek).sum() / weights[kept].sum())
    R = float(l64_row.max() - l64_row[kept].min())
    return (2 * mean_E / temperature * math.exp(2 * float(Ek.max()) / temperature)
            + 2 * gamma(V) + 2 * (R / temperature + 3) * U + 2 * U)


def midpoints(F, kept, tol):
    """(tokens, u): every kept token whose CDF interval is wider than 4*tol,
    with the midpoint of that interval."""
    lo = torch.cat([F.new_zeros(1), F[:-1]])
    wide = kept & ((F - lo) > 4 * tol)
    toks = wide.nonzero().squeeze(1)
    return toks, ((lo + F) / 2)[toks]
