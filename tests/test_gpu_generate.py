"""AWDLSTM.generate and InferenceWrapper.predict on the native path: the
device-side feedback loop against a hand-stepped loop that reads every id to
the host, for the LSTM and the QRNN encoder."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_WORDS = 64


def _vocab():
    from code_intelligence_amd.text.tokenizer import Vocab, defaults_specials
    return Vocab(defaults_specials + [f"w{i}" for i in range(500)])


_MODELS = {}


def _lm(qrnn):
    """The tiny bf16 config of test_serve_batched_equals_single_gpu."""
    if qrnn not in _MODELS:
        from code_intelligence_amd.models.awd_lstm import AWDLSTM
        torch.manual_seed(0)
        m = AWDLSTM(vocab_sz=len(_vocab()), emb_sz=64, n_hid=96, n_layers=2,
                    qrnn=qrnn)
        m.decoder.decoder.bias.data.normal_(0, 0.5)
        _MODELS[qrnn] = m.to(device=DEV, dtype=torch.bfloat16).eval()
    return _MODELS[qrnn]


def _prompt():
    return torch.tensor([[12, 40, 7, 300, 21], [9, 9, 15, 100, 508],
                         [50, 51, 52, 53, 54]], device=DEV)


@pytest.mark.parametrize("qrnn", [False, True], ids=["lstm", "qrnn"])
def test_generate_equals_hand_stepped_loop(qrnn):
    from code_intelligence_amd.ops import sample_next
    m = _lm(qrnn)
    prompt = _prompt()
    B = prompt.size(0)
    us = torch.rand(N_WORDS, B, generator=torch.Generator().manual_seed(1))
    ids, logp = m.generate(prompt, N_WORDS, temperature=0.8, min_p=0.001,
                           uniforms=us)
    assert ids.shape == (B, N_WORDS) and ids.dtype == torch.int64
    assert logp.shape == (B, N_WORDS) and logp.dtype == torch.float32
    lin = m.decoder.decoder
    want, want_lp, x = [], [], prompt
    with torch.no_grad():
        m.reset(B)
        for step in range(N_WORDS):
            h = m.encoder(x)[1][-1][:, -1]
            nxt, lp = sample_next(h, lin.weight, lin.bias, us[step].to(DEV),
                                  0.8, 0.001, 0)
            want.append(nxt.cpu().tolist())          # host read every word
            want_lp.append(lp.cpu().tolist())
            x = torch.tensor(want[-1], device=DEV).unsqueeze(1)
    assert ids.t().cpu().tolist() == want
    assert logp.t().cpu().tolist() == want_lp
    assert bool(((ids > 0) & (ids < len(_vocab()))).all())


@pytest.mark.parametrize("qrnn", [False, True], ids=["lstm", "qrnn"])
def test_seed_reproducible_no_unk_and_flags_restored(qrnn):
    m = _lm(qrnn)
    prompt = _prompt()
    m.train()
    m.encoder.rnns[0].eval()
    flags = [mod.training for mod in m.modules()]
    try:
        a, _ = m.generate(prompt, N_WORDS, seed=3)
        assert [mod.training for mod in m.modules()] == flags
    finally:
        m.eval()
    b, _ = m.generate(prompt, N_WORDS, seed=3)
    c, _ = m.generate(prompt, N_WORDS, seed=4)
    assert torch.equal(a, b)               # eval mode inside: dropout is off
    assert not torch.equal(a, c)
    assert not bool((a == 0).any()) and not bool((c == 0).any())
    # with unk pushed far above everything else it is still never drawn, and
    # is drawn once the filter is off
    lin = m.decoder.decoder
    old = lin.bias.data[0].clone()
    lin.bias.data[0] = 30.0
    try:
        d, _ = m.generate(prompt, N_WORDS, seed=5)
        e, _ = m.generate(prompt, 4, seed=5, no_unk=False)
    finally:
        lin.bias.data[0] = old
    assert not bool((d == 0).any()) and bool((e == 0).all())


def test_wrapper_predict_on_decoder_artifact(tmp_path):
    from code_intelligence_amd.engine.inference import (InferenceWrapper,
                                                        save_artifacts)
    m = _lm(False)
    save_artifacts(m, _vocab(), tmp_path / "art", with_decoder=True)
    w = InferenceWrapper(model_path=str(tmp_path / "art"), device=DEV)
    text = "w1 w2 w3 w4 w5 w6"
    out = w.predict(text, 5, seed=2)
    assert out.startswith(text + " ")
    # w<i> tokens carry no caps or repetition markers most of the time; a
    # marker only ever shortens the text by merging into its neighbour
    assert 1 <= len(out[len(text) + 1:].split(" ")) <= 5
    assert out == w.predict(text, 5, seed=2)
    many = w.predict(text, 5, seed=2, n_samples=4)
    assert len(many) == 4 and all(s.startswith(text + " ") for s in many)
    plain = InferenceWrapper(encoder=m.encoder, vocab=_vocab(), device=DEV)
    with pytest.raises(RuntimeError, match="with_decoder=True"):
        plain.predict(text, 5)
