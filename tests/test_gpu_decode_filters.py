"""decode_cutoff (decode.hip) and the filtered sample_next against the fp64
rule of decode_filter_ref.py.

decode_cutoff is checked on the kernel's own fp32 logits, the reference being
computed in fp64 from those same fp32 values, so no GEMV error enters.

top-k is a count: the cutoff must be the k-th largest fp32 logit bit for bit
(-inf for k >= |C|: nothing filters).

top-p compares S(x) = sum_{l >= x} exp(l - max) with top_p * S(min), every sum
in fp32. With u = 2^-24:
  tol = 2*gamma(n) + 2*(R + 3)*u + 2u        (decode_filter_ref.cutoff_tol)
bounds |S(x) / S(min) - F(x)| plus the rounding of top_p and of the product:
each weight is within (R + 3)u relative (l - max rounds once on a value <= R,
expf is within an ulp), a sum of positive terms is within gamma(n) relative
with n the longest chain of additions a term passes through, both twice for
the ratio. The kernel's chains, for a row of V entries:
  * a histogram pass adds a thread's entries of one bin in ascending order,
    at most ceil(V / 1024) - 1 additions, then 6 butterfly levels, then the
    16 waves in ascending order (15), then the walk down the 14 bins onto the
    carried sum (14): ceil(V / 1024) + 34 per pass, of which only the 14 of
    the walk repeat in a later pass;
  * the bisection in LDS adds at most 7 entries per thread, 6 levels, 15
    waves and the carried sum: 28, on top of the passes' walks.
  With P passes n <= ceil(V / 1024) + 20 + 14 * P + 28. A row of at most
  7168 entries takes exactly one pass: n = ceil(V / 1024) + 62. Two passes at
  least halve the key span of the bracket, so P <= 64 always and
  n = ceil(V / 1024) + 944 holds for any row. Only an addition of two
  non-zero operands rounds, and a sum of V terms has at most V - 1 of those,
  so n = V holds as well; the test uses the smaller of the two.
top_p is the midpoint of two consecutive normalised cumulative sums of the
reference, so it is half the boundary token's probability away from both; the
test asserts that this exceeds 2 * tol and then requires the exact cutoff.
"""
import math

import pytest
import torch

from decode_ref import (U, cdf, cdf_tol, gamma, inputs, logits_ref, midpoints)
from decode_filter_ref import (NEG_INF, cutoff_ref, cutoff_tol,
                               filtered_weights, midpoint_top_p, nucleus_cdf,
                               sorted_candidates)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNK = 0
SPIKES = {7: 3.0, 300: 2.5}
SHAPES = [
    (1, 37, 20, torch.float32),
    (3, 1000, 264, torch.bfloat16),
    (11, 513, 264, torch.bfloat16),
]
IDS = ["1x37x20-fp32", "3x1000x264-bf16", "11x513x264-bf16"]
LONG_V = 66003                       # past the 60 * 1024 register-cached entries


def _lib():
    from code_intelligence_amd.ops import extension as ext
    return ext.require()


def n_chain(V):
    return min(V, (V + 1023) // 1024 + (62 if V <= 7168 else 944))


_CASES = {}


def _case(shape):
    if shape not in _CASES:
        from code_intelligence_amd.ops import decode_logits
        B, V, H, dtype = shape
        spikes = {i % V: off for i, off in SPIKES.items()}
        h, w, bias = inputs(B, V, H, dtype, True, seed=5, spikes=spikes)
        l64, E = logits_ref(h, w, bias)
        dev = [t.to(DEV) for t in (h, w, bias)]
        logits, partials = decode_logits(*dev)
        torch.cuda.synchronize()
        _CASES[shape] = dict(h=h, w=w, bias=bias, l64=l64, E=E, dev=dev,
                             logits=logits, partials=partials,
                             l32=logits.cpu())
    return _CASES[shape]


def _long_row():
    if "long" not in _CASES:
        g = torch.Generator().manual_seed(11)
        l32 = (3.0 * torch.randn(1, LONG_V, generator=g)).float()
        _CASES["long"] = dict(l32=l32, logits=l32.to(DEV))
    return _CASES["long"]


def _cutoff(logits, k, top_p, unk):
    out = torch.full((logits.size(0),), 7.0, device=DEV)
    _lib().decode_cutoff(logits.contiguous(), k, top_p, unk, out)
    torch.cuda.synchronize()
    return out.cpu()


def _same_bits(got, want):
    return torch.equal(got.view(torch.int32),
                       torch.tensor(want, dtype=torch.float32).view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_top_k_cutoff_is_the_kth_largest_bit_for_bit(shape):
    B, V, H, dtype = shape
    c = _case(shape)
    nC = V - 1
    for k in (1, 2, 64, nC - 1, nC, nC + 5):
        got = _cutoff(c["logits"], k, 0.0, UNK)
        want = [cutoff_ref(c["l32"][b], k, None, UNK)[0] for b in range(B)]
        assert _same_bits(got, want), (k, got, want)
        if k < nC:
            srt = [sorted_candidates(c["l32"][b], UNK)[0] for b in range(B)]
            assert want == [float(s[k - 1]) for s in srt]
        else:
            assert want == [NEG_INF] * B


def test_top_k_keeps_every_entry_tied_with_the_kth():
    c = _case(SHAPES[1])
    row = c["l32"][0].clone()
    vals, idx = sorted_candidates(row, UNK)
    k = 5
    for j in idx[100:103].tolist():          # three copies of the k-th value
        row[j] = float(vals[k - 1])
    for kk in (k, k + 1, k + 3):
        got = _cutoff(row.unsqueeze(0).to(DEV), kk, 0.0, UNK)
        want, kept = cutoff_ref(row, kk, None, UNK)
        assert _same_bits(got, [want]) and want == float(vals[k - 1])
        assert int(kept.sum()) == k + 3
    got = _cutoff(row.unsqueeze(0).to(DEV), k + 4, 0.0, UNK)
    assert float(got[0]) < float(vals[k - 1])


def _check_top_p(l32_row, dev_row, unk, targets, V):
    vals, _ = sorted_candidates(l32_row, unk)
    F = nucleus_cdf(vals)
    tol = cutoff_tol(vals, n_chain(V))
    for target in targets:
        top_p, want, margin = midpoint_top_p(vals, F, target)
        print(f"target {target}: top_p={top_p:.6f} margin/tol={margin / tol:.1f}")
        assert margin > 2 * tol, (target, margin, tol)
        ref, _ = cutoff_ref(l32_row, None, top_p, unk)
        assert ref == want
        got = _cutoff(dev_row, 0, top_p, unk)
        assert _same_bits(got, [want]), (target, float(got[0]), want)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_top_p_cutoff_at_midpoints_bit_for_bit(shape):
    B, V, H, dtype = shape
    c = _case(shape)
    for b in range(B):
        _check_top_p(c["l32"][b], c["logits"][b:b + 1], UNK, (0.1, 0.5, 0.9), V)


def test_long_row_rereads_through_l2():
    c = _long_row()
    row = c["l32"][0]
    _check_top_p(row, c["logits"], UNK, (0.1, 0.5), LONG_V)
    vals, _ = sorted_candidates(row, UNK)
    for k in (1, 50, 30000, LONG_V - 2):
        got = _cutoff(c["logits"], k, 0.0, UNK)
        assert _same_bits(got, [float(vals[k - 1])]), k
    # both filters: the larger cutoff wins
    top_p, want_p, _ = midpoint_top_p(vals, nucleus_cdf(vals), 0.5)
    got = _cutoff(c["logits"], 50, top_p, UNK)
    assert _same_bits(got, [max(want_p, float(vals[49]))])


def test_edge_rows():
    one = torch.tensor([[1.5]], device=DEV)
    assert _same_bits(_cutoff(one, 1, 0.5, -1), [1.5])
    assert _same_bits(_cutoff(one, 0, 1.0, -1), [1.5])
    assert _same_bits(_cutoff(one, 3, 0.0, -1), [NEG_INF])
    assert _same_bits(_cutoff(one, 1, 0.5, 0), [NEG_INF])    # no candidate
    # unk is the arg-max: it counts for nothing
    row = torch.tensor([[0.5, 9.0, -1.0, 0.25, 0.5]], device=DEV)
    assert _same_bits(_cutoff(row, 1, 0.0, 1), [0.5])
    assert _same_bits(_cutoff(row, 3, 0.0, 1), [0.25])
    assert _same_bits(_cutoff(row, 1, 0.0, -1), [9.0])
    want, _ = cutoff_ref(row[0].cpu(), None, 0.6, 1)
    assert want == 0.5 and _same_bits(_cutoff(row, 0, 0.6, 1), [0.5])
    # the draw with no candidate is what it is without a cutoff
    from code_intelligence_amd.ops import sample_next
    h, w = torch.ones(1, 4, device=DEV), torch.ones(1, 4, device=DEV)
    u = torch.tensor([0.3], device=DEV)
    a = sample_next(h, w, None, u, unk_idx=0)
    b = sample_next(h, w, None, u, unk_idx=0, top_k=1, top_p=0.5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- sample_next end to end -------------------------------------------------
def _gap_ok(l64, E, kept, unk):
    """The fp64 logit gap across the cutoff exceeds the two bounds E."""
    out = ~kept
    if unk >= 0:
        out[unk] = False
    if not bool(out.any()):
        return True
    lo_in = l64.masked_fill(~kept, float("inf")).argmin()
    hi_out = l64.masked_fill(~out, NEG_INF).argmax()
    return float(l64[lo_in] - l64[hi_out]) > float(E[lo_in] + E[hi_out])


# the spikes (7 and 300) are the two best candidates: filters that cut right
# below them leave a logit gap far wider than the GEMV bounds
@pytest.mark.parametrize("filt", [(2, None), (None, 0.01), (64, 0.01),
                                  (2, 0.9)],
                         ids=["k2", "p0.01", "k64-p0.01", "k2-p0.9"])
@pytest.mark.parametrize("shape", SHAPES[1:], ids=IDS[1:])
def test_filtered_draws_match_fp64(shape, filt):
    from code_intelligence_amd.ops import sample_next
    B, V, H, dtype = shape
    top_k, target = filt
    c = _case(shape)
    hd, wd, bd = c["dev"]
    for b in range(B):
        l64, E = c["l64"][b], c["E"][b]
        top_p = None
        if target is not None:
            vals, _ = sorted_candidates(l64, UNK)
            top_p, _, margin = midpoint_top_p(vals, nucleus_cdf(vals), target)
            # the logit error moves the normalised mass like the CDF's
            assert margin > 2 * cdf_tol(E, l64, torch.ones(V, dtype=torch.bool),
                                        torch.softmax(l64, 0), V, 1.0)
        p64, kept, wts = filtered_weights(l64, UNK, top_k, top_p, None, 0.8)
        assert _gap_ok(l64, E, kept, UNK)
        assert kept.nonzero().squeeze(1).tolist() == [7, 300]
        F = cdf(wts)
        tol = cdf_tol(E, l64, kept, wts, V, 0.8)
        toks, us = midpoints(F, kept, tol)
        n_kept = int(kept.sum())
        print(f"row {b}: kept={n_kept} tested={len(toks)} tol={tol:.3e}")
        assert len(toks) >= 0.5 * n_kept, (len(toks), n_kept)
        edge = torch.tensor([0.0, math.nextafter(1.0, 0.0)], dtype=torch.float64)
        us = torch.cat([us, edge])
        N = len(us)
        ids, logp = sample_next(hd[b:b + 1].expand(N, -1).contiguous(), wd, bd,
                                us.to(DEV), temperature=0.8, unk_idx=UNK,
                                top_k=top_k, top_p=top_p)
        ids, logp = ids.cpu(), logp.double().cpu()
        assert torch.equal(ids[:-2], toks)
        assert bool(kept[ids].all())
        E_lse = float(E.max()) + gamma(V + 2)
        want = torch.log(p64[ids])
        assert float(((logp - want).abs() / (E[ids] + E_lse)).max()) <= 1.0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_no_filter_is_the_parent_call_bit_for_bit(shape):
    from code_intelligence_amd.ops import sample_next
    B, V, H, dtype = shape
    c = _case(shape)
    hd, wd, bd = c["dev"]
    u = torch.rand(B, generator=torch.Generator().manual_seed(2)).to(DEV)
    ids = torch.empty(B, dtype=torch.int64, device=DEV)
    logp = torch.empty(B, device=DEV)
    _lib().decode_sample(c["logits"], c["partials"], u, 0.8, 1e-3, UNK, ids,
                         logp)
    for kw in ({}, dict(top_k=None, top_p=None), dict(top_p=1.0)):
        got_ids, got_lp = sample_next(hd, wd, bd, u, 0.8, 1e-3, UNK, **kw)
        assert torch.equal(got_ids, ids)
        assert torch.equal(got_lp.view(torch.int32), logp.view(torch.int32))


def test_host_checks():
    lib = _lib()
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
    with pytest.raises(RuntimeError, match="top_p"):
        lib.decode_cutoff(z(2, 100), 0, 1.5, -1, z(2))
    with pytest.raises(RuntimeError, match="top_k"):
        lib.decode_cutoff(z(2, 100), -1, 0.5, -1, z(2))
    with pytest.raises(RuntimeError, match="unk"):
        lib.decode_cutoff(z(2, 100), 1, 0.5, 100, z(2))
    with pytest.raises(RuntimeError, match="out must be"):
        lib.decode_cutoff(z(2, 100), 1, 0.5, -1, z(3))
    with pytest.raises(RuntimeError, match="cut must be"):
        lib.decode_sample(z(2, 100), z(2, 2, 2), z(2), 1.0, 0.0, -1,
                          z(2, dtype=torch.int64), z(2), z(3))
