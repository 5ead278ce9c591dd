"""TextClassifier.predict_proba (streamed pool + fused head) against
sigmoid(model.eval()(ids, lengths)) on the GPU kernel path.

Both paths run the same encoder calls on the same chunks, so they see the
same fp32 hidden states; they differ in the order of the fp32 window sum
(per-chunk partials vs one pass) and in the head (BatchNorm folded into one
fused launch vs the unfused modules). Each is within its own forward-error
bound of the exact fp64 head on the exact fp64 pool of those hidden states
(pool_head_ref.head_bounds, derived in test_gpu_pool_stream.py):

  mean features : n <= max_len fp32 additions in any order and one division
                  leave each within gamma(n) * mean|x| of the exact mean;
                  that enters as the first layer's input error.
  streamed path : gamma(K + 4) per layer, as for the kernel alone.
  forward path  : gamma(K + 9): the unfused BatchNorm rounds x - mean,
                  var + eps, rsqrt, * invstd, * gamma, + beta (6), the GEMM
                  its products, K - 1 additions and the bias add.
  sigmoid       : E / 4 + 4u each.

So |p_stream - p_forward| <= (E_s + E_f) / 4 + 8u, and the streamed logits
and probabilities are also checked against the exact ones with E_s alone.
"""
import copy

import pytest
import torch

from pool_head_ref import U, gamma, head_bounds

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NO_DROP = dict(output_p=0.0, hidden_p=0.0, input_p=0.0, embed_p=0.0,
               weight_p=0.0)
T, BPTT, MAX_LEN = 19, 4, 6
# windows start at [13, 0, 1, 6]: row 0's misses chunks 0-2 (left to the
# kernel, since row 1 needs chunk 0), a partial last chunk, a length-1 row
LENS = [19, 1, 7, 12]
# windows start at [13, 9, 11, 6]: the encoder skips chunk [0, 4) outright
LENS_SKIP = [19, 15, 17, 12]


def _model(qrnn, lin_ftrs=(50,), ps=(0.0,)):
    from code_intelligence_amd.models.classifier import get_text_classifier
    torch.manual_seed(3)
    cfg = dict(emb_sz=16, n_hid=24, n_layers=2, pad_token=1, qrnn=qrnn,
               **NO_DROP)
    m = get_text_classifier(50, 3, bptt=BPTT, max_len=MAX_LEN, config=cfg,
                            lin_ftrs=lin_ftrs, ps=ps)
    g = torch.Generator().manual_seed(9)
    for bn in m.head.layers:
        if isinstance(bn, torch.nn.BatchNorm1d):
            n = bn.num_features
            bn.running_mean.copy_(torch.randn(n, generator=g) * 0.3)
            bn.running_var.copy_(0.5 + torch.rand(n, generator=g))
            bn.weight.data.copy_(0.5 + torch.rand(n, generator=g))
            bn.bias.data.copy_(0.3 * torch.randn(n, generator=g))
    return m.to(DEV)


def _batch(lens=LENS):
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(2, 50, (len(lens), T), generator=g)
    for b, l in enumerate(lens):
        ids[b, l:] = 1
    return ids.to(DEV), torch.tensor(lens, device=DEV)


def _exact_features(model, ids, lens):
    """fp64 [mean, max, last] of the hidden states forward pools, and the
    absolute error an fp32 mean may carry."""
    with torch.no_grad():
        hidden, rel = model[0](ids, lens)
    h = hidden.double().cpu()
    B, _, H = h.shape
    f = torch.zeros(B, 3 * H, dtype=torch.float64)
    ferr = torch.zeros_like(f)
    for b, l in enumerate(rel.tolist()):
        lo = max(0, l - MAX_LEN)
        win = h[b, lo:l]
        f[b, :H] = win.mean(0)
        f[b, H:2 * H] = win.max(0).values
        f[b, 2 * H:] = h[b, l - 1]
        ferr[b, :H] = gamma(l - lo) * win.abs().mean(0)
    return f, ferr


@pytest.mark.parametrize("lens,kept", [(LENS, 5), (LENS_SKIP, 4)],
                         ids=["len1-row", "skipped-chunk"])
@pytest.mark.parametrize("qrnn", [False, True], ids=["lstm", "qrnn"])
def test_predict_proba_matches_forward(qrnn, lens, kept):
    model = _model(qrnn).eval()
    ids, lens = _batch(lens)
    with torch.no_grad():
        before = model(ids, lens)
    model.train()
    probs, logits = model.predict_proba(ids, lens)
    assert model.training, "training flag must be restored"
    assert model[0].max_live_chunks == 1
    model.eval()
    probs_eval, _ = model.predict_proba(ids, lens)
    assert not model.training
    assert torch.equal(probs, probs_eval)
    with torch.no_grad():
        after = model(ids, lens)
    assert torch.equal(before, after), "forward changed by predict_proba"
    assert model[0].kept_chunks == kept

    f, ferr = _exact_features(model, ids, lens)
    head = copy.deepcopy(model.head).cpu()
    z, Es = head_bounds(head, f, ferr, roundings=4)
    _, Ef = head_bounds(head, f, ferr, roundings=9)
    exact = torch.sigmoid(z)
    p_s = probs.double().cpu()
    p_f = torch.sigmoid(before).double().cpu()
    xs = float(((p_s - exact).abs() / (Es / 4 + 4 * U)).max())
    xl = float(((logits.double().cpu() - z).abs() / Es).max())
    xd = float(((p_s - p_f).abs() / ((Es + Ef) / 4 + 8 * U)).max())
    print(f"stream prob err/bound={xs:.3f} logit err/bound={xl:.3f} "
          f"stream-vs-forward/bound={xd:.3f}")
    assert probs.dtype == torch.float32 and probs.shape == (4, 3)
    assert xs <= 1.0 and xl <= 1.0, (xs, xl)
    assert xd <= 1.0, xd


def test_softmax_rows_sum_to_one():
    model = _model(False).eval()
    ids, lens = _batch()
    probs, logits = model.predict_proba(ids, lens, multi_label=False)
    assert float((probs.double().sum(1) - 1).abs().max()) <= 3 * 2.0 ** -23
    assert torch.equal(probs.argmax(1), logits.argmax(1))


def test_three_layer_head_takes_the_torch_fallback_and_matches():
    """Both sides run the unfused modules (gamma(K + 9) per layer) on mean
    features that each carry the gamma(n) * mean|x| error."""
    from code_intelligence_amd.models.classifier import fold_head_bn
    model = _model(False, lin_ftrs=(20, 10), ps=(0.0, 0.0)).eval()
    assert fold_head_bn(model.head) is None
    ids, lens = _batch()
    with torch.no_grad():
        ref = model(ids, lens)
    probs, logits = model.predict_proba(ids, lens)
    assert model[0].max_live_chunks == 1
    f, ferr = _exact_features(model, ids, lens)
    _, E = head_bounds(copy.deepcopy(model.head).cpu(), f, ferr, roundings=9)
    xl = float(((logits - ref).abs().double().cpu() / (2 * E)).max())
    xp = float(((probs - torch.sigmoid(ref)).abs().double().cpu()
                / (2 * E / 4 + 8 * U)).max())
    print(f"fallback logits/bound={xl:.3f} probs/bound={xp:.3f}")
    assert xl <= 1.0 and xp <= 1.0, (xl, xp)


def test_fold_cache_is_dropped_by_train_and_load_state_dict():
    model = _model(False).eval()
    ids, lens = _batch()
    p0, _ = model.predict_proba(ids, lens)
    assert model._folded is not None
    cached = model._folded
    model.predict_proba(ids, lens)
    assert model._folded is cached, "fold recomputed between eval calls"
    sd = copy.deepcopy(model.state_dict())
    sd["1.layers.0.running_mean"] += 1.0
    model.load_state_dict(sd)
    assert model._folded is None
    p1, _ = model.predict_proba(ids, lens)
    assert not torch.equal(p0, p1)
    model.train()
    assert model._folded is None


def test_peak_memory_does_not_grow_with_document_length():
    """Doubling T (window = whole document, so ``forward`` keeps every
    chunk) must not raise predict_proba's peak allocation: a retained chunk
    costs at least one chunk of final-layer states, B * bptt * H * 4 bytes,
    per extra chunk, so growth below ONE such chunk means none is retained.
    ``forward`` on the same inputs must grow by at least the T extra
    positions of final-layer states it concatenates."""
    from code_intelligence_amd.models.classifier import get_text_classifier
    B, H, bptt, T1 = 8, 64, 16, 128
    torch.manual_seed(3)
    cfg = dict(emb_sz=H, n_hid=96, n_layers=2, pad_token=1, qrnn=False,
               **NO_DROP)
    model = get_text_classifier(50, 3, bptt=bptt, max_len=4 * T1, config=cfg,
                                ps=(0.0,)).to(DEV).eval()
    chunk_bytes = B * bptt * H * 4

    def peak_above_inputs(fn, T):
        ids = torch.randint(2, 50, (B, T), device=DEV)
        lens = torch.full((B,), T, device=DEV)
        out = None
        for _ in range(2):                     # first call warms workspaces
            del out
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = fn(ids, lens)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
        return peak

    def fwd(ids, lens):
        with torch.no_grad():
            return model(ids, lens)

    stream = [peak_above_inputs(model.predict_proba, T) for T in (T1, 2 * T1)]
    full = [peak_above_inputs(fwd, T) for T in (T1, 2 * T1)]
    print(f"peak above inputs: predict_proba {stream}, forward {full}, "
          f"one chunk {chunk_bytes}")
    assert stream[1] - stream[0] < chunk_bytes, stream
    assert full[1] - full[0] >= B * T1 * H * 4, full
