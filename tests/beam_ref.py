"""fp64 references and error bounds shared by the beam-search tests.

``fastai_beam_search`` is a literal transcription of fastai 1.x
``LanguageLearner.beam_search``: ``log_softmax``, ``unk`` to -inf, ``topk``,
``argsort``, ``torch.cat`` of the node prefixes, ``select_hidden``. The only
change is that both sorts are stable, which pins fastai's unspecified tie
order to the documented one (lower vocabulary index, lower flat index).
"""
import torch

U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


def stable_topk(x, k):
    """(values, indices) of the k largest per row, ties to the lower index."""
    order = torch.sort(x, dim=1, descending=True, stable=True).indices[:, :k]
    return x.gather(1, order), order


def fastai_beam_search(model, prompt, n_words, top_k, beam_sz, no_unk=True,
                       unk_idx=0):
    """(nodes (B, n_words), scores (B,)): the surviving beams without the
    prompt, ascending score order. The model is left in eval mode."""
    model.eval()
    model.reset(1)
    xb = prompt.clone()
    nodes = xb.clone()
    scores = torch.zeros(1, dtype=model.decoder.decoder.weight.dtype)
    with torch.no_grad():
        for _ in range(n_words):
            out = torch.log_softmax(model(xb)[0][:, -1], dim=-1)
            if no_unk:
                out[:, unk_idx] = -float("inf")
            values, indices = stable_topk(out, top_k)
            scores = (-values + scores[:, None]).view(-1)
            n = nodes.size(0)
            indices_idx = torch.arange(0, n)[:, None].expand(
                n, top_k).contiguous().view(-1)
            sort_idx = torch.sort(scores, stable=True).indices[:beam_sz]
            scores = scores[sort_idx]
            nodes = torch.cat(
                [nodes[:, None].expand(n, top_k, nodes.size(1)),
                 indices[:, :, None].expand(n, top_k, 1)], dim=2)
            nodes = nodes.view(-1, nodes.size(2))[sort_idx]
            model[0].select_hidden(indices_idx[sort_idx])
            xb = nodes[:, -1][:, None]
    return nodes[:, prompt.size(1):], scores


def rescore(model, prompt, nodes):
    """Score of every beam from scratch: one batch-1 pass over prompt + beam,
    minus the summed log-probabilities of the beam's tokens."""
    model.eval()
    T = prompt.size(1)
    out = []
    with torch.no_grad():
        for row in nodes:
            model.reset(1)
            seq = torch.cat([prompt[0], row[:-1]]).unsqueeze(0)
            lp = torch.log_softmax(model(seq)[0][0, T - 1:], dim=-1)
            out.append(-lp.gather(1, row.unsqueeze(1)).sum())
    return torch.stack(out)


def topk_ref(logits, k, unk):
    """fp64 top-k log-probabilities of the given (already rounded) tensor."""
    x = logits.double().cpu()
    lse = torch.logsumexp(x, dim=1, keepdim=True)
    keys = x.clone()
    if unk >= 0:
        keys[:, unk] = -float("inf")
    _, idx = stable_topk(keys, k)
    return x.gather(1, idx) - lse, idx, lse.squeeze(1)


def topk_val_tol(x64, lse64, vals64):
    """Per-entry bound on |kernel value - fp64 value| (B,k); derivation in
    test_gpu_beam.py."""
    V = x64.size(1)
    R = (x64.max(dim=1).values - x64.min(dim=1).values)
    nres = -(-V // 64) + 9
    e_s = gamma(V + 2) + (R + 2) * U + (R + 3 * nres) * U
    log_s = (lse64 - x64.max(dim=1).values).abs()
    e_lse = e_s + 2 * U * log_s + U * lse64.abs()
    return e_lse.unsqueeze(1) + U * vals64.abs()
