"""CPU side of beam search: AWDLSTM.beam_search against a literal transcription
of fastai's loop on tiny fp64 models, the QRNN prev_x reordering against
re-encoding every beam from scratch, the tie rules and limits of
topk_logprobs / beam_select, and the InferenceWrapper round trip."""
import pytest
import torch

from beam_ref import fastai_beam_search, rescore

from code_intelligence_amd.engine.inference import InferenceWrapper, save_artifacts
from code_intelligence_amd.models.awd_lstm import AWDLSTM
from code_intelligence_amd.ops import beam_select, topk_logprobs
from code_intelligence_amd.text.tokenizer import Vocab, defaults_specials


def _tiny_lm(qrnn, dtype=torch.float64, vocab_sz=64):
    torch.manual_seed(0)
    m = AWDLSTM(vocab_sz=vocab_sz, emb_sz=16, n_hid=24, n_layers=2, qrnn=qrnn)
    m.decoder.decoder.bias.data.normal_(0, 0.5)
    return m.to(dtype)


PROMPT = torch.tensor([[5, 9, 12]])


@pytest.mark.parametrize("beam_sz", [6, 100], ids=["cut", "growth-only"])
@pytest.mark.parametrize("qrnn", [False, True], ids=["lstm", "qrnn"])
def test_beam_search_matches_the_fastai_loop_fp64(qrnn, beam_sz):
    m = _tiny_lm(qrnn).train()
    m.encoder.rnns[0].eval()               # a mixed set of flags to restore
    flags = [mod.training for mod in m.modules()]
    ids, nodes, scores = m.beam_search(PROMPT, 5, top_k=3, beam_sz=beam_sz,
                                       uniform=0.0)
    assert [mod.training for mod in m.modules()] == flags
    want_nodes, want_scores = fastai_beam_search(m, PROMPT, 5, 3, beam_sz)
    n = min(beam_sz, 3 ** 5)
    assert nodes.shape == (n, 5) and nodes.dtype == torch.int64
    assert ids.shape == (5,) and ids.dtype == torch.int64
    assert torch.equal(nodes, want_nodes)
    # two fp64 evaluation orders (log_softmax vs l - logsumexp, the decoder
    # on (B,T,H) vs on the last position): a few ulp of ~15 per word
    assert torch.allclose(scores, want_scores, rtol=0, atol=1e-12)
    assert bool((scores[1:] >= scores[:-1]).all())
    assert not bool((nodes == 0).any())
    assert torch.equal(ids, nodes[0])      # u = 0 takes the best beam


def test_qrnn_prev_x_follows_the_beams():
    """Layer 0 of the QRNN encoder (window 2) reads the previous token's
    embedding from prev_x. Unless select_hidden reorders it, a beam continues
    from another beam's last token and its score no longer equals the score
    of its own sequence."""
    m = _tiny_lm(True)
    _, nodes, scores = m.beam_search(PROMPT, 5, top_k=3, beam_sz=6)
    # parents are permuted at some step, or the test shows nothing
    assert len({tuple(r[:-1]) for r in nodes.tolist()}) > 1
    assert torch.allclose(scores, rescore(m, PROMPT, nodes), rtol=0, atol=1e-10)


def test_select_hidden_keeps_a_same_shape_prev_x_buffer():
    m = _tiny_lm(True)
    enc = m.encoder
    m.eval()
    with torch.no_grad():
        enc.reset(3)
        enc(torch.tensor([[5], [9], [12]]))
    buf = enc.rnns[0].prev_x
    want = buf.clone()[[2, 0, 0]]
    enc.select_hidden(torch.tensor([2, 0, 0]))
    assert enc.rnns[0].prev_x is buf and torch.equal(buf, want)
    enc.select_hidden(torch.tensor([1, 2]))
    assert enc.bs == 2 and torch.equal(enc.rnns[0].prev_x, want[[1, 2]])
    assert all(h.size(0) == 2 and c.size(0) == 2 for h, c in enc.hidden)


def test_final_draw_is_an_inverse_cdf_over_the_beams():
    m = _tiny_lm(False)
    _, nodes, scores = m.beam_search(PROMPT, 4, top_k=3, beam_sz=5)
    for temperature in (1.0, 0.5):
        p = torch.softmax(-scores / temperature, 0)
        F = p.cumsum(0)
        lo = torch.cat([F.new_zeros(1), F[:-1]])
        for b in range(5):
            ids, _, _ = m.beam_search(PROMPT, 4, top_k=3, beam_sz=5,
                                      temperature=temperature,
                                      uniform=float((lo[b] + F[b]) / 2))
            assert torch.equal(ids, nodes[b])
    a = m.beam_search(PROMPT, 4, top_k=3, beam_sz=5, seed=3)[0]
    assert torch.equal(a, m.beam_search(PROMPT, 4, top_k=3, beam_sz=5, seed=3)[0])
    picks = {tuple(m.beam_search(PROMPT, 4, top_k=3, beam_sz=5, seed=s)[0]
                   .tolist()) for s in range(12)}
    assert len(picks) > 1


def test_topk_tie_rule_and_unk():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0, 2.0, 2.0],
                      [2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]], dtype=torch.float64)
    vals, idx = topk_logprobs(x, 4)
    assert idx.tolist() == [[1, 2, 4, 5], [0, 1, 2, 3]]
    lp = torch.log_softmax(x, dim=1)
    assert torch.allclose(vals, lp.gather(1, idx), rtol=0, atol=1e-14)
    vals, idx = topk_logprobs(x, 4, unk_idx=2)
    assert idx.tolist() == [[1, 4, 5, 6], [0, 1, 3, 4]]
    # unk stays in the softmax
    assert torch.allclose(vals, lp.gather(1, idx), rtol=0, atol=1e-14)
    vals, idx = topk_logprobs(x, 6, unk_idx=6)
    assert idx.tolist() == [[1, 2, 4, 5, 0, 3], [0, 1, 2, 3, 4, 5]]


def test_beam_select_tie_rule():
    scores = torch.tensor([0.5, 0.5, 0.0], dtype=torch.float64)
    vals = torch.tensor([[-1.0, -1.0], [-1.0, -2.0], [-1.5, -2.5]],
                        dtype=torch.float64)
    idx = torch.tensor([[7, 8], [9, 10], [11, 12]])
    s, parent, token = beam_select(scores, vals, idx, 4)
    # candidates 1.5 1.5 | 1.5 2.5 | 1.5 2.5: equal scores in flat order
    assert s.tolist() == [1.5, 1.5, 1.5, 1.5]
    assert parent.tolist() == [0, 0, 1, 2] and token.tolist() == [7, 8, 9, 11]
    s, parent, token = beam_select(scores, vals, idx, 100)
    assert parent.tolist() == [0, 0, 1, 2, 1, 2]
    assert token.tolist() == [7, 8, 9, 11, 10, 12]
    out = (torch.zeros(2, 5, dtype=torch.float64)[1, :4],
           torch.zeros(4, dtype=torch.int64), torch.zeros(8, dtype=torch.int64)[::2])
    got = beam_select(scores, vals, idx, 4, out=out)
    assert got[0] is out[0] and out[2].tolist() == [7, 8, 9, 11]


def test_limits_raise_value_error():
    x = torch.zeros(2, 10, dtype=torch.float64)
    for k, unk in [(0, -1), (65, -1), (11, -1), (10, 0)]:
        with pytest.raises(ValueError, match="k"):
            topk_logprobs(x, k, unk)
    assert topk_logprobs(x, 10)[1].shape == (2, 10)
    assert topk_logprobs(x, 9, 9)[1].shape == (2, 9)
    for unk in (-2, 10):
        with pytest.raises(ValueError, match="unk_idx"):
            topk_logprobs(x, 3, unk)
    with pytest.raises(ValueError, match="k"):
        topk_logprobs(torch.zeros(1, 100), 65)
    vals = torch.zeros(1025, 16)
    idx = torch.zeros(1025, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match="16400"):
        beam_select(torch.zeros(1025), vals, idx, 1000)
    with pytest.raises(ValueError, match="beam_sz"):
        beam_select(torch.zeros(2), vals[:2], idx[:2], 0)
    with pytest.raises(ValueError, match="scores"):
        beam_select(torch.zeros(3), vals[:2], idx[:2], 4)
    m = _tiny_lm(False, torch.float32)
    with pytest.raises(ValueError, match="prompt_ids"):
        m.beam_search(torch.tensor([[1, 2], [3, 4]]), 2)
    with pytest.raises(ValueError, match="top_k"):
        m.beam_search(PROMPT, 2, top_k=64)      # 64 > V - 1 candidates
    with pytest.raises(ValueError, match="exceed 16384"):
        m.beam_search(PROMPT, 4, top_k=20, beam_sz=1000)
    with pytest.raises(ValueError, match="temperature"):
        m.beam_search(PROMPT, 2, temperature=0.0)


# ---- artifacts -------------------------------------------------------------
def _vocab():
    return Vocab(defaults_specials + [f"w{i}" for i in range(55)])


def test_wrapper_beam_search_round_trip(tmp_path):
    m = _tiny_lm(False, torch.float32)
    vocab = _vocab()
    save_artifacts(m, vocab, tmp_path / "a", with_decoder=True)
    w = InferenceWrapper(model_path=str(tmp_path / "a"), device="cpu")
    text = "w1 w2 w3"
    out = w.beam_search(text, 5, top_k=4, beam_sz=20, seed=11)
    assert out.startswith(text + " ")
    assert out == w.beam_search(text, 5, top_k=4, beam_sz=20, seed=11)
    ids, _, _ = m.beam_search(torch.tensor([vocab.numericalize(text.split())]),
                              5, top_k=4, beam_sz=20, seed=11)
    raw = w.beam_search(text, 5, top_k=4, beam_sz=20, seed=11, sep="|",
                        decoder=list)
    assert raw == text + "|" + "|".join(vocab.itos[i] for i in ids.tolist())
    assert "xxunk" not in raw
    assert w.beam_search("", 2, beam_sz=5, seed=1).startswith(" ")
    # the embedding path of the same wrapper still works
    assert w.get_pooled_features(text).shape == (1, 48)
    save_artifacts(m, vocab, tmp_path / "b")
    plain = InferenceWrapper(model_path=str(tmp_path / "b"), device="cpu")
    with pytest.raises(RuntimeError, match="with_decoder=True"):
        plain.beam_search(text, 3)
