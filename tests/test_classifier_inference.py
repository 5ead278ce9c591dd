"""Serving the fine-tuned classifier on the CPU reference path: the streamed
pool against ``forward``, the artifact round trip, ClassifierInferenceWrapper,
the label model and its route through IssueLabelPredictor, and the CLI's
``--export_dir``."""
import copy
import json
import sys
import weakref
from pathlib import Path

import numpy as np
import pytest
import torch

from code_intelligence_amd.engine.classifier_inference import (
    ClassifierInferenceWrapper, save_classifier_artifacts)
from code_intelligence_amd.models.classifier import (fold_head_bn,
                                                     get_text_classifier)
from code_intelligence_amd.ops.pool import StreamingConcatPool, pool_head
from code_intelligence_amd.text.tokenizer import Tokenizer, Vocab

sys.path.insert(0, str(Path(__file__).resolve().parent))
from pool_head_ref import U, gamma, head_bounds  # noqa: E402

NO_DROP = dict(output_p=0.0, hidden_p=0.0, input_p=0.0, embed_p=0.0,
               weight_p=0.0)
LABELS = ["bug", "docs", "io"]
TEXTS = [
    "crash in module when saving a file",
    "docs typo",
    "the reader fails on a large file and then the writer crashes too, "
    "every time, with the same trace as before",
    "question about saving",
    "io error",
]


def tiny(qrnn=False, n_class=3, vocab_sz=50, bptt=4, max_len=6, lin_ftrs=(7,)):
    torch.manual_seed(1)
    cfg = dict(emb_sz=8, n_hid=12, n_layers=2, pad_token=1, qrnn=qrnn,
               **NO_DROP)
    m = get_text_classifier(vocab_sz, n_class, bptt=bptt, max_len=max_len,
                            config=cfg, lin_ftrs=lin_ftrs,
                            ps=(0.0,) * len(lin_ftrs))
    g = torch.Generator().manual_seed(2)
    for bn in m.head.layers:
        if isinstance(bn, torch.nn.BatchNorm1d):
            n = bn.num_features
            bn.running_mean.copy_(torch.randn(n, generator=g) * 0.3)
            bn.running_var.copy_(0.5 + torch.rand(n, generator=g))
            bn.weight.data.copy_(0.5 + torch.rand(n, generator=g))
            bn.bias.data.copy_(0.3 * torch.randn(n, generator=g))
    return m.eval()


def _batch(lens, T=19):
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(2, 50, (len(lens), T), generator=g)
    for b, l in enumerate(lens):
        ids[b, l:] = 1
    return ids, torch.tensor(lens)


# --- streamed pool vs forward -------------------------------------------------
@pytest.mark.parametrize("lens", [[19, 1, 7, 12], [19, 15, 17, 12]],
                         ids=["len1-row", "skipped-chunk"])
@pytest.mark.parametrize("qrnn", [False, True], ids=["lstm", "qrnn"])
def test_streaming_cpu_path_matches_forward_in_float64(qrnn, lens):
    """``forward`` itself cannot run in float64 (its CPU pool sums in fp32
    and the head pins itself to fp32), so the float64 comparison is with
    forward's own pieces: the hidden states ``model[0]`` returns, pooled over
    the same windows and fed to the unfused head, all in float64. The literal
    fp32 ``forward`` is then compared at fp32 accuracy."""
    model = tiny(qrnn).double()
    ids, lengths = _batch(lens)
    with torch.no_grad():
        hidden, rel = model[0](ids, lengths)
    assert hidden.dtype == torch.float64
    B, _, H = hidden.shape
    want = torch.zeros(B, 3 * H, dtype=torch.float64)
    for b, l in enumerate(rel.tolist()):
        win = hidden[b, max(0, l - 6):l]
        want[b] = torch.cat([win.mean(0), win.max(0).values, hidden[b, l - 1]])
    pool = model[0].stream_pool(ids, lengths, dtype=torch.float64)
    assert model[0].max_live_chunks == 1
    got = pool.features()
    assert got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-10

    head64 = copy.deepcopy(model.head.layers).double()
    with torch.no_grad():
        want_logits = head64(want.clone())
    probs, logits = pool_head(pool.state, pool.lengths, pool.max_len,
                              *[t.double() for t in fold_head_bn(model.head)])
    # evaluated in float64, the folded head differs from the unfolded one by
    # the single fp32 rounding of each folded weight and bias: gamma(1) * A
    # per layer (pool_head_ref), plus float64 noise far below 1e-12
    z, E = head_bounds(model.head, want, terms=1)
    assert float((z - want_logits).abs().max()) <= 1e-12
    assert bool(((logits - want_logits).abs() <= E + 1e-12).all())
    assert bool(((probs - torch.sigmoid(want_logits)).abs()
                 <= E / 4 + 1e-12).all())


def _exact_on_own_hidden(model, ids, lengths, max_len=6):
    """fp64 [mean, max, last] of the fp32 hidden states ``forward`` pools and
    the error an fp32 mean of n terms may carry, gamma(n) * mean|x|."""
    with torch.no_grad():
        hidden, rel = model[0](ids, lengths)
    h = hidden.double()
    B, _, H = h.shape
    f = torch.zeros(B, 3 * H, dtype=torch.float64)
    ferr = torch.zeros_like(f)
    for b, l in enumerate(rel.tolist()):
        lo = max(0, l - max_len)
        win = h[b, lo:l]
        f[b] = torch.cat([win.mean(0), win.max(0).values, h[b, l - 1]])
        ferr[b, :H] = gamma(l - lo) * win.abs().mean(0)
    return f, ferr


@pytest.mark.parametrize("lin_ftrs", [(7,), (7, 5)], ids=["folded", "fallback"])
@pytest.mark.parametrize("qrnn", [False, True], ids=["lstm", "qrnn"])
def test_fp32_predict_proba_matches_forward_within_derived_bound(qrnn, lin_ftrs):
    """The bound of test_gpu_classifier_predict.py on the CPU path: both
    routes see the same fp32 hidden states; the streamed route is within
    E(K+4) (folded) or E(K+9) (unfused fallback) of the exact fp64 head on
    their exact pool, ``forward`` within E(K+9)."""
    model = tiny(qrnn, lin_ftrs=lin_ftrs)
    ids, lengths = _batch([19, 1, 7, 12])
    with torch.no_grad():
        ref = model(ids, lengths)
    probs, logits = model.predict_proba(ids, lengths)
    assert probs.dtype == torch.float32
    f, ferr = _exact_on_own_hidden(model, ids, lengths)
    z, Es = head_bounds(model.head, f, ferr,
                        roundings=4 if len(lin_ftrs) == 1 else 9)
    _, Ef = head_bounds(model.head, f, ferr, roundings=9)
    assert bool(((logits.double() - z).abs() <= Es).all())
    assert bool(((ref.double() - z).abs() <= Ef).all())
    assert bool(((probs.double() - torch.sigmoid(ref).double()).abs()
                 <= (Es + Ef) / 4 + 8 * U).all())


def test_previous_chunk_is_dead_when_the_next_encoder_call_starts():
    """Independent of the model's own counter: every tensor an encoder call
    returned must be unreferenced by the time the next call starts, and
    ``max_live_chunks`` must report a chunk that is held on to."""
    model = tiny()
    ids, lengths = _batch([19, 1, 7, 12])
    enc = model.encoder
    inner = enc.forward
    refs, alive_at_start = [], []

    def probe(x, *a, **k):
        alive_at_start.append(sum(r() is not None for r in refs))
        del refs[:]
        raw, out = inner(x, *a, **k)
        refs.extend(weakref.ref(t) for t in raw + out)
        return raw, out

    enc.forward = probe
    try:
        model.predict_proba(ids, lengths)
        assert len(alive_at_start) == 5 and alive_at_start == [0] * 5
        assert model[0].max_live_chunks == 1

        held = []

        def hoarder(x, *a, **k):
            raw, out = inner(x, *a, **k)
            held.append(out[-1])
            return raw, out

        enc.forward = hoarder
        model.predict_proba(ids, lengths)
        assert model[0].max_live_chunks == 2
    finally:
        del enc.forward


def test_non_finite_padding_outside_the_window_is_never_read():
    h = torch.randn(2, 6, 3, dtype=torch.float64)
    lens = torch.tensor([6, 2])
    clean = StreamingConcatPool(2, 3, 4, "cpu", torch.float64)
    clean.update(h, lens, 0)
    h[0, :2] = float("nan")                   # before row 0's window [2, 6)
    h[1, 2:] = float("inf")                   # row 1's padding
    dirty = StreamingConcatPool(2, 3, 4, "cpu", torch.float64)
    dirty.update(h[:, :3], lens, 0)
    dirty.update(h[:, 3:], lens, 3)
    assert torch.isfinite(dirty.state).all()
    assert torch.allclose(dirty.state, clean.state, rtol=0, atol=1e-14)


def test_streaming_pool_chunk_past_lengths_and_missed_rows_cpu():
    h = torch.randn(3, 10, 4, dtype=torch.float64)
    lens = torch.tensor([10, 1, 4])
    pool = StreamingConcatPool(3, 4, 3, "cpu", torch.float64)
    pool.state[:] = 7.5
    pool.update(h[:, :2], lens, 0)            # only row 1 ([0,1)) and row 2 ([1,4))
    assert bool((pool.state[0] == 7.5).all())
    assert torch.equal(pool.state[1, 8:], h[1, 0])
    before = pool.state.clone()
    pool.update(h, lens, 10)
    assert torch.equal(pool.state, before)


def test_predict_proba_restores_mode_and_leaves_forward_alone():
    model = tiny()
    ids, lengths = _batch([19, 1, 7, 12])
    with torch.no_grad():
        before = model(ids, lengths)
    p_eval, _ = model.predict_proba(ids, lengths)
    # gradual unfreezing: root training, frozen groups individually in eval
    model.train()
    model.encoder.encoder.eval()
    model.encoder.rnns[0].eval()
    flags = {n: m.training for n, m in model.named_modules()}
    assert not all(flags.values()) and any(flags.values())
    p_mixed, _ = model.predict_proba(ids, lengths)
    assert {n: m.training for n, m in model.named_modules()} == flags
    assert torch.equal(p_mixed, p_eval)
    # root in eval, a head BatchNorm left in train mode: eval is still forced
    # (running statistics, as the folded head assumes) and the flag returns
    model.eval()
    bn = model.head.layers[0]
    bn.train()
    mean0 = bn.running_mean.clone()
    p_bn, _ = model.predict_proba(ids, lengths)
    assert bn.training and not model.training
    assert torch.equal(bn.running_mean, mean0)
    assert torch.equal(p_bn, p_eval)
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(ids, lengths), before)


# --- artifact + wrapper -------------------------------------------------------
@pytest.fixture(scope="module")
def vocab():
    return Vocab.create(Tokenizer().process_all(TEXTS), min_freq=1)


@pytest.fixture(scope="module")
def artifact(tmp_path_factory, vocab):
    root = tmp_path_factory.mktemp("clas")
    model = tiny(vocab_sz=len(vocab))
    save_classifier_artifacts(model, vocab, LABELS, root,
                              thresholds={"bug": 0.3, "io": None})
    return root, model


def test_artifact_round_trip(artifact, vocab):
    root, model = artifact
    cfg = json.loads((root / "config.json").read_text())
    assert cfg == {"emb_sz": 8, "n_hid": 12, "n_layers": 2, "qrnn": False,
                   "bptt": 4, "max_len": 6, "lin_ftrs": [7], "n_class": 3,
                   "multi_label": True, "classifier_file": "classifier.pth"}
    assert json.loads((root / "labels.json").read_text()) == LABELS
    assert json.loads((root / "thresholds.json").read_text()) == \
        {"bug": 0.3, "io": None}
    sd = torch.load(root / "classifier.pth", weights_only=True)
    assert set(sd) == set(model.state_dict())
    w = ClassifierInferenceWrapper(str(root), device="cpu")
    assert w.labels == LABELS and len(w.vocab) == len(vocab)
    for (n, a), (_, b) in zip(model.state_dict().items(),
                              w.model.state_dict().items()):
        assert torch.equal(a, b), n
    direct = ClassifierInferenceWrapper(model=copy.deepcopy(model), vocab=vocab,
                                        labels=LABELS, device="cpu")
    assert np.array_equal(w.predict(TEXTS[0])[2], direct.predict(TEXTS[0])[2])


def test_predict_tuple(artifact):
    root, _ = artifact
    w = ClassifierInferenceWrapper(str(root), device="cpu")
    names, mask, probs = w.predict(TEXTS[2])
    assert isinstance(names, list) and all(isinstance(n, str) for n in names)
    assert mask.shape == (3,) and mask.dtype == bool
    assert probs.shape == (3,) and probs.dtype == np.float32
    assert ((probs > 0) & (probs < 1)).all()
    want = [probs[0] >= 0.3, probs[1] >= 0.5, False]      # io: None = never
    assert mask.tolist() == want
    assert names == [l for l, m in zip(LABELS, want) if m]


def test_predict_batch_equals_predict_and_ignores_order(artifact):
    root, _ = artifact
    w = ClassifierInferenceWrapper(str(root), device="cpu")
    single = np.stack([w.predict(t)[2] for t in TEXTS])
    batch = w.predict_batch(TEXTS, bs=2)
    assert batch.shape == (len(TEXTS), 3) and batch.dtype == np.float32
    # padding adds encoder steps after a row's window only; the batched
    # GEMMs may still round differently from the single-row ones
    assert np.abs(batch - single).max() <= 1e-6
    perm = [3, 0, 4, 2, 1]
    shuffled = w.predict_batch([TEXTS[i] for i in perm], bs=2)
    assert np.array_equal(shuffled, batch[perm])


def test_empty_text_and_token_cap(artifact, monkeypatch):
    root, _ = artifact
    w = ClassifierInferenceWrapper(str(root), device="cpu")
    unk = w.vocab.stoi["xxunk"]
    assert w.numericalize("") == [unk]
    _, _, p_empty = w.predict("")
    assert np.isfinite(p_empty).all()
    assert np.array_equal(w.predict_batch(["", TEXTS[0]])[0], p_empty)
    monkeypatch.setenv("CI_SERVE_MAX_TOKENS", "3")
    assert len(w.numericalize(TEXTS[2])) == 3
    capped = w.predict(TEXTS[2])[2]
    assert np.array_equal(w.predict_batch([TEXTS[2]])[0], capped)
    monkeypatch.setenv("CI_SERVE_MAX_TOKENS", "0")
    assert len(w.numericalize(TEXTS[2])) > 3
    assert not np.array_equal(w.predict(TEXTS[2])[2], capped)


# --- label service ------------------------------------------------------------
def test_label_model_thresholds(artifact):
    from code_intelligence_amd.label.finetuned_classifier_model import (
        FineTunedClassifierLabelModel)
    root, _ = artifact
    m = FineTunedClassifierLabelModel.from_path(str(root), device="cpu")
    assert m.thresholds == {"bug": 0.3, "io": None}
    title, text = "crash when saving", ["the writer crashes", "same trace"]
    doc = m.build_document(title, text)
    assert doc == m.wrapper.process_dict(
        {"title": title, "body": "the writer crashes\nsame trace"})["text"]
    probs = dict(zip(LABELS, m.wrapper.predict(doc)[2]))
    m.thresholds = {"bug": 0.0, "docs": 0.0, "io": 0.0}
    got = m.predict_issue_labels("o", "r", title, text)
    assert got == {k: pytest.approx(float(v)) for k, v in probs.items()}
    m.thresholds = {"bug": float(probs["bug"]), "docs": 1.1, "io": None}
    assert set(m.predict_issue_labels("o", "r", title, text)) == {"bug"}
    m.thresholds = {"bug": None, "io": None}             # docs: default 0.5
    assert set(m.predict_issue_labels("o", "r", title, text)) == \
        ({"docs"} if probs["docs"] >= 0.5 else set())


class _Universal:
    def predict_issue_labels(self, org, repo, title, text, context=None):
        return {"kind/question": 0.9}


def test_predictor_routes_finetuned_classifier_kind(artifact):
    from code_intelligence_amd.label.combined_model import CombinedLabelModels
    from code_intelligence_amd.label.finetuned_classifier_model import (
        FineTunedClassifierLabelModel)
    from code_intelligence_amd.label.issue_label_predictor import (
        IssueLabelPredictor)
    root, _ = artifact
    p = IssueLabelPredictor(universal=_Universal())
    p._load_one({"kind": "finetuned_classifier", "path": str(root),
                 "org": "acme", "repo": "tool", "device": "cpu"})
    p._load_one({"kind": "finetuned_classifier", "path": str(root),
                 "org": "acme", "device": "cpu"})
    assert set(p.models) == {"universal", "acme/tool_combined", "acme_combined"}
    combined = p.models["acme/tool_combined"]
    assert isinstance(combined, CombinedLabelModels)
    assert isinstance(combined.models[-1], FineTunedClassifierLabelModel)
    assert p._model_for("acme", "tool") is combined
    assert p._model_for("acme", "other") is p.models["acme_combined"]
    combined.models[-1].thresholds = {l: 0.0 for l in LABELS}
    out = p.predict({"repo_owner": "acme", "repo_name": "tool",
                     "title": "crash when saving", "text": ["trace"]})
    assert set(out) == {"kind/question", *LABELS}
    with pytest.raises(ValueError, match="unknown model kind"):
        p._load_one({"kind": "nope", "org": "acme"})


# --- CLI ----------------------------------------------------------------------
def _cli_inputs(tmp_path):
    from code_intelligence_amd.engine.inference import save_artifacts
    from code_intelligence_amd.models.awd_lstm import AWDLSTM
    texts = [f"crash in module{i % 3} when saving file number {i}"
             for i in range(10)]
    vocab = Vocab.create(Tokenizer().process_all(texts), min_freq=1)
    torch.manual_seed(0)
    lm = AWDLSTM(vocab_sz=len(vocab), emb_sz=8, n_hid=12, n_layers=2)
    save_artifacts(lm, vocab, tmp_path / "lm")
    rows = [{"text": t, "labels": ["bug"] + (["io"] if i % 2 else [])}
            for i, t in enumerate(texts)]
    (tmp_path / "d.jsonl").write_text("\n".join(json.dumps(r) for r in rows))
    return texts, ["--artifacts", str(tmp_path / "lm"),
                   "--data", str(tmp_path / "d.jsonl"), "--bs", "4",
                   "--bptt", "5", "--max_len", "7", "--device", "cpu",
                   "--valid_pct", "0.2"]


def test_finetune_cli_export_dir(tmp_path, capsys):
    from code_intelligence_amd.train import finetune_cli
    texts, argv = _cli_inputs(tmp_path)
    plain = finetune_cli.main(argv + ["--out", str(tmp_path / "a.pth")])
    plain_stdout = capsys.readouterr().out
    exported = finetune_cli.main(argv + ["--out", str(tmp_path / "b.pth"),
                                         "--export_dir", str(tmp_path / "clas")])
    assert capsys.readouterr().out == plain_stdout
    assert exported == plain
    # without the flag: the same files as before, and nothing else
    assert sorted(f.name for f in tmp_path.iterdir()) == [
        "a.pth", "a.pth.labels.json", "b.pth", "b.pth.labels.json", "clas",
        "d.jsonl", "lm"]
    a = torch.load(tmp_path / "a.pth", weights_only=True)
    b = torch.load(tmp_path / "b.pth", weights_only=True)
    for k in a["model"]:
        assert torch.equal(a["model"][k], b["model"][k]), k

    assert sorted(f.name for f in (tmp_path / "clas").iterdir()) == [
        "classifier.pth", "config.json", "labels.json", "vocab.json"]
    cfg = json.loads((tmp_path / "clas" / "config.json").read_text())
    assert (cfg["bptt"], cfg["max_len"], cfg["n_class"]) == (5, 7, 2)
    w = ClassifierInferenceWrapper(str(tmp_path / "clas"), device="cpu")
    assert w.labels == ["bug", "io"]
    for k, v in w.model.state_dict().items():
        assert torch.equal(v, b["model"][k]), k
    names, mask, probs = w.predict(texts[0])
    assert probs.shape == (2,) and np.isfinite(probs).all()
    assert w.predict_batch(texts).shape == (10, 2)
