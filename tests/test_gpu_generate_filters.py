"""AWDLSTM.generate with top_k / top_p on the native path against the fp64 rule.

The loop is re-stepped by hand with the ids generate returned, so the encoder
state, and with it every decoder input h, has generate's bits. Each word is
then decided in fp64 on the host from that h and the bf16 weights
(decode_ref.logits_ref, decode_filter_ref.filtered_weights). A draw is
compared only where fp32 cannot change it:
  * the fp64 logit gap across the cutoff exceeds the two logit bounds E, and
    the nucleus mass at both ends of the boundary run is further than
    2 * cdf_tol from top_p, so the kept set is the reference's;
  * u is further than 2 * cdf_tol from both ends of the chosen token's CDF
    interval.
Other draws are skipped and counted; at most half may be (the cover rule of
test_gpu_decode.py). Where only the first condition holds the id must still
lie in the reference set.
"""
import pytest
import torch

from decode_ref import cdf, cdf_tol, logits_ref
from decode_filter_ref import (NEG_INF, filtered_weights, group_ends,
                               nucleus_cdf, sorted_candidates)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V, B, N_WORDS = 505, 3, 6
TOP_K, TOP_P, TEMP = 5, 0.9, 0.8

_MODEL = []


def _lm():
    if not _MODEL:
        from code_intelligence_amd.models.awd_lstm import AWDLSTM
        torch.manual_seed(0)
        m = AWDLSTM(vocab_sz=V, emb_sz=24, n_hid=48, n_layers=2)
        m.decoder.decoder.bias.data.normal_(0, 0.5)
        _MODEL.append(m.to(device=DEV, dtype=torch.bfloat16).eval())
    return _MODEL[0]


def _prompt():
    return torch.tensor([[12, 40, 7, 300, 21], [9, 9, 15, 100, 504],
                         [50, 51, 52, 53, 54]], device=DEV)


def _decoder_inputs(m, ids):
    """h of every word, the loop fed with ``ids``."""
    hs, x = [], _prompt()
    with torch.no_grad():
        m.reset(B)
        for step in range(ids.size(1)):
            hs.append(m.encoder(x)[1][-1][:, -1].clone())
            x = ids[:, step:step + 1]
    return hs


def _set_is_certain(l64, E, kept, top_p, mass_tol):
    out = ~kept
    out[0] = False                                       # unk
    lo_in = l64.masked_fill(~kept, float("inf")).argmin()
    hi_out = l64.masked_fill(~out, NEG_INF).argmax()
    if not float(l64[lo_in] - l64[hi_out]) > float(E[lo_in] + E[hi_out]):
        return False
    vals, _ = sorted_candidates(l64, 0)
    Fe = nucleus_cdf(vals)[group_ends(vals)]
    return float((Fe - top_p).abs().min()) > 2 * mass_tol


def test_generate_top_k_top_p_matches_fp64():
    m = _lm()
    lin = m.decoder.decoder
    us = torch.rand(N_WORDS, B, generator=torch.Generator().manual_seed(1))
    ids, logp = m.generate(_prompt(), N_WORDS, temperature=TEMP, uniforms=us,
                           top_k=TOP_K, top_p=TOP_P)
    assert ids.shape == (B, N_WORDS) and not bool((ids == 0).any())
    hs = _decoder_inputs(m, ids)
    w, bias = lin.weight.detach().cpu(), lin.bias.detach().cpu()
    ids = ids.cpu()
    skipped = 0
    for step in range(N_WORDS):
        l64, E = logits_ref(hs[step].cpu(), w, bias)
        for b in range(B):
            p64, kept, wts = filtered_weights(l64[b], 0, TOP_K, TOP_P, None, TEMP)
            assert 1 <= int(kept.sum()) <= TOP_K
            tol = cdf_tol(E[b], l64[b], kept, wts, V, TEMP)
            mass_tol = cdf_tol(E[b], l64[b], torch.ones(V, dtype=torch.bool),
                               p64, V, 1.0)
            if not _set_is_certain(l64[b], E[b], kept, TOP_P, mass_tol):
                skipped += 1
                continue
            got = int(ids[b, step])
            assert bool(kept[got]), (step, b, got)
            F = cdf(wts)
            lo = torch.cat([F.new_zeros(1), F[:-1]])
            u = float(us[step, b])
            want = int((F > u).nonzero()[0])
            if min(u - float(lo[want]), float(F[want]) - u) <= 2 * tol:
                skipped += 1
                continue
            assert got == want, (step, b, got, want)
    print(f"skipped {skipped} of {B * N_WORDS} draws")
    assert skipped <= B * N_WORDS // 2, skipped


def test_generate_top_k_one_is_the_arg_max():
    m = _lm()
    lin = m.decoder.decoder
    ids, _ = m.generate(_prompt(), N_WORDS, seed=1, top_k=1)
    again, _ = m.generate(_prompt(), N_WORDS, seed=2, top_k=1, temperature=3.0)
    assert torch.equal(ids, again)
    hs = _decoder_inputs(m, ids)
    w, bias = lin.weight.detach().cpu(), lin.bias.detach().cpu()
    from code_intelligence_amd.ops import sample_next
    for step in range(N_WORDS):
        h = hs[step].cpu()
        l64, E = logits_ref(h, w, bias)
        l64[:, 0] = NEG_INF
        top2 = l64.topk(2, dim=1)
        gap = top2.values[:, 0] - top2.values[:, 1]
        assert bool((gap > E.gather(1, top2.indices).sum(dim=1)).all())
        cpu_ids, _ = sample_next(h.double(), w.double(), bias.double(),
                                 torch.zeros(B, dtype=torch.float64),
                                 unk_idx=0, top_k=1)
        assert torch.equal(cpu_ids, top2.indices[:, 0])
        assert torch.equal(ids[:, step].cpu(), cpu_ids), step
