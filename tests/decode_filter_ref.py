"""fp64 reference of the top-k / nucleus rule of ops/decode.py, by sorting the
candidates and an explicit cumulative sum. Helpers shared by the filter tests;
the unfiltered machinery is decode_ref.py's.
"""
import torch

from decode_ref import U, gamma

NEG_INF = float("-inf")


def sorted_candidates(l_row, unk):
    """(values descending, their vocabulary indices) of every index but unk."""
    idx = torch.arange(l_row.numel())
    if unk >= 0:
        idx = idx[idx != unk]
    vals, order = l_row[idx].double().sort(descending=True, stable=True)
    return vals, idx[order]


def nucleus_cdf(vals):
    """Normalised running sums of exp(l - max) down the sorted candidates, an
    explicit cumsum in fp64."""
    w = torch.exp(vals - vals[0]).tolist()
    F, acc = [], 0.0
    for x in w:
        acc += x
        F.append(acc)
    return torch.tensor(F, dtype=torch.float64) / acc


def cutoff_ref(l_row, top_k, top_p, unk):
    """(cutoff, kept mask) of one row: max(t_k, t_p), -inf where nothing
    filters, and K = {v != unk : l_v >= cutoff}."""
    l_row = l_row.double()
    V = l_row.numel()
    cand = torch.ones(V, dtype=torch.bool)
    if unk >= 0:
        cand[unk] = False
    cut = NEG_INF
    if int(cand.sum()) > 0:
        vals, _ = sorted_candidates(l_row, unk)
        n = vals.numel()
        if top_k is not None and top_k < n:
            cut = max(cut, float(vals[top_k - 1]))
        if top_p is not None and top_p < 1.0:
            F = nucleus_cdf(vals)
            # mass{l >= vals[i]} is F at the end of vals[i]'s run of ties; the
            # first i with F[i] >= top_p starts the run that is t_p
            at = min(int((F < top_p).sum()), n - 1)
            cut = max(cut, float(vals[at]))
    return cut, cand & (l_row >= cut)


def group_ends(vals):
    """Indices i at which a run of equal sorted values ends."""
    last = torch.ones(vals.numel(), dtype=torch.bool)
    last[:-1] = vals[:-1] > vals[1:]
    return last.nonzero().squeeze(1)


def midpoint_top_p(vals, F, target):
    """(top_p, cutoff value, margin): top_p is the midpoint between the two
    consecutive run-end values of F nearest ``target``; the cutoff is then
    the value of the run that ends at the upper one, and margin is half that
    run's probability."""
    ends = group_ends(vals)
    Fe = F[ends]
    g = int((Fe - target).abs().argmin())
    g = max(g, 1)                       # needs a run above it
    lo, hi = float(Fe[g - 1]), float(Fe[g])
    return (lo + hi) / 2, float(vals[ends[g]]), (hi - lo) / 2


def cutoff_tol(vals, n_chain):
    """2*gamma(n) + 2*(R + 3)*u + 2u: decode_ref.cdf_tol without the logit
    error; R = max - min candidate logit, n the longest chain of additions."""
    R = float(vals[0] - vals[-1])
    return 2 * gamma(n_chain) + 2 * (R + 3) * U + 2 * U


def filtered_weights(l64_row, unk, top_k, top_p, min_p, temperature):
    """(p64, kept mask, weights): decode_ref.fastai_weights with min_p
    applied inside the top-k / nucleus set."""
    p = torch.softmax(l64_row, dim=0)
    _, keep = cutoff_ref(l64_row, top_k, top_p, unk)
    res = torch.where(keep, p, torch.zeros_like(p))
    if min_p is not None and bool((res >= min_p).any()):
        res = torch.where(res < min_p, torch.zeros_like(res), res)
    kept = res > 0
    return p, kept, res.pow(1.0 / temperature)
