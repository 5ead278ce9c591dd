"""Classifier fine-tuning (models/classifier.py, train/classifier.py) on
the CPU reference path: layer groups, discriminative learning rates,
freezing, checkpoint keys, chunked-encoder equivalence and a tiny fit."""
import json
import math

import pytest
import torch

from code_intelligence_amd.models.awd_lstm import AWDLSTM
from code_intelligence_amd.models.classifier import (
    TextClassifier, awd_lstm_clas_config, get_text_classifier)
from code_intelligence_amd.ops.pool import _cpu_concat_pool
from code_intelligence_amd.train.classifier import (ClassifierTrainer,
                                                    PaddedBatchLoader)

NO_DROP = dict(output_p=0.0, hidden_p=0.0, input_p=0.0, embed_p=0.0,
               weight_p=0.0)


def tiny(n_layers=2, n_class=3, qrnn=False, bptt=8, max_len=10, **kw):
    cfg = dict(emb_sz=16, n_hid=32, n_layers=n_layers, pad_token=1,
               qrnn=qrnn, **NO_DROP)
    cfg.update(kw)
    return get_text_classifier(50, n_class, bptt=bptt, max_len=max_len,
                               config=cfg, ps=(0.0,))


# --- lr_range ---------------------------------------------------------------

def test_lr_range_three_forms_on_six_groups():
    tr = ClassifierTrainer(tiny(n_layers=4))
    assert len(tr.groups) == 6
    assert tr.lr_range(3e-3) == [3e-3] * 6
    assert tr.lr_range(slice(4e-4)) == [4e-5] * 5 + [4e-4]
    lrs = tr.lr_range(slice(1e-5, 1e-3))
    assert lrs[0] == pytest.approx(1e-5) and lrs[-1] == pytest.approx(1e-3)
    ratios = [b / a for a, b in zip(lrs, lrs[1:])]
    assert all(r == pytest.approx(100 ** 0.2) for r in ratios)


# --- freezing ---------------------------------------------------------------

def _trainable(model):
    return {n for n, p in model.named_parameters() if p.requires_grad}


def test_freeze_levels_toggle_expected_parameters():
    model = tiny(n_layers=3)
    tr = ClassifierTrainer(model)
    names = {n for n, _ in model.named_parameters()}
    head = {n for n in names if n.startswith("1.")}
    last_rnn = {n for n in names if n.startswith("0.module.rnns.2.")}
    assert head and last_rnn
    tr.freeze()
    assert _trainable(model) == head
    tr.freeze_to(-2)
    assert _trainable(model) == head | last_rnn
    tr.unfreeze()
    assert _trainable(model) == names
    # one optimizer group per layer group, covering every parameter once
    assert len(tr.opt.param_groups) == len(tr.groups) == 5
    n_opt = sum(len(g["params"]) for g in tr.opt.param_groups)
    assert n_opt == len(list(model.parameters()))


def test_frozen_step_changes_only_the_head():
    torch.manual_seed(0)
    model = tiny()
    tr = ClassifierTrainer(model)
    tr.freeze()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    ids = torch.randint(2, 50, (5, 12))
    lens = torch.tensor([12, 9, 5, 1, 12])
    y = (torch.rand(5, 3) < 0.5).float()
    model.train()
    tr.train_step(ids, lens, y, tr.lr_range(1e-2))
    for n, p in model.named_parameters():
        changed = not torch.equal(p, before[n])
        assert changed == n.startswith("1."), n


# --- checkpoints ------------------------------------------------------------

def test_state_dict_keys_and_encoder_round_trip(tmp_path):
    model = tiny()
    keys = set(model.state_dict())
    for k in ("0.module.encoder.weight", "0.module.rnns.0.weight_hh_l0_raw",
              "1.layers.6.weight"):
        assert k in keys, k
    assert isinstance(model, TextClassifier)
    assert model[0].module is model.encoder and model[1] is model.head
    torch.manual_seed(1)
    lm = AWDLSTM(vocab_sz=50, emb_sz=16, n_hid=32, n_layers=2)
    lm.save_encoder(tmp_path / "enc.pth")
    model.load_encoder(tmp_path / "enc.pth")
    want = lm.encoder.state_dict()
    got = model.encoder.state_dict()
    assert set(want) == set(got)
    for k in want:
        assert torch.equal(want[k], got[k]), k


def test_lm_config_builds_and_head_stays_fp32():
    from code_intelligence_amd.models.awd_lstm import awd_lstm_lm_config
    cfg = dict(awd_lstm_lm_config)
    cfg.update(emb_sz=16, n_hid=32, n_layers=2)
    minus = dict(cfg)
    minus.pop("tie_weights"); minus.pop("out_bias")   # what the notebook passes
    for c in (cfg, minus):
        m = get_text_classifier(50, 4, config=c, lin_ftrs=(20,), ps=(0.2,))
        assert m.head.layers[2].in_features == 48
        assert m.head.layers[6].out_features == 4
        assert m.head.layers[1].p == cfg["output_p"]
        assert m.head.layers[5].p == 0.2
    m = m.to(torch.bfloat16)
    assert m.encoder.encoder.weight.dtype == torch.bfloat16
    assert all(t.dtype == torch.float32 for t in m.head.state_dict().values()
               if t.is_floating_point())
    assert get_text_classifier(50, 2).encoder.emb_sz == awd_lstm_clas_config["emb_sz"]


# --- MultiBatchEncoder ------------------------------------------------------

def _naive_logits(model, ids, lengths):
    """Every chunk with grad, batch-major cat, windowed CPU composition."""
    mbe = model[0]
    enc = mbe.module
    enc.reset(ids.size(0))
    outs = []
    for s in range(0, ids.size(1), mbe.bptt):
        _, o = enc(ids[:, s:s + mbe.bptt])
        outs.append(o[-1])
    pooled = _cpu_concat_pool(torch.cat(outs, dim=1), lengths, mbe.max_len)
    return model[1](pooled.float())


# lengths, kept chunks for T=24, bptt=8, max_len=10:
#   mixed: lo = [14,10,3,0,14] -> g = 0, nothing dropped
#   long : lo = [14,12,10,9,14] -> g = 9 >= bptt, chunk [0,8) is dropped
LENGTHS = {"mixed": ([24, 20, 13, 9, 24], 3), "long": ([24, 22, 20, 19, 24], 2)}


@pytest.mark.parametrize("qrnn", [False, True], ids=["lstm", "qrnn"])
@pytest.mark.parametrize("case", ["mixed", "long"])
def test_multibatch_encoder_matches_naive(case, qrnn):
    lens_l, kept = LENGTHS[case]
    torch.manual_seed(4)
    model = tiny(qrnn=qrnn)
    model.train()
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(2, 50, (5, 24), generator=g)
    lens = torch.tensor(lens_l)
    for b, l in enumerate(lens_l):
        ids[b, l:] = 1
    y = (torch.rand(5, 3, generator=g) < 0.5).float()
    lossf = torch.nn.BCEWithLogitsLoss()

    def grads(fn):
        model.zero_grad(set_to_none=True)
        loss = lossf(fn(model, ids, lens), y)
        loss.backward()
        return float(loss.detach()), {n: p.grad.clone() for n, p in
                             model.named_parameters() if p.grad is not None}

    l_ref, g_ref = grads(_naive_logits)
    l_got, g_got = grads(lambda m, i, l: m(i, l))
    assert model[0].kept_chunks == kept
    assert abs(l_ref - l_got) < 1e-6
    assert set(g_ref) == set(g_got) == {n for n, _ in model.named_parameters()}
    for n in g_ref:
        assert (g_ref[n] - g_got[n]).abs().max() < 1e-6, n
    rnn_w = "0.module.rnns.0.weight_raw" if qrnn \
        else "0.module.rnns.0.weight_hh_l0_raw"
    assert g_got[rnn_w].abs().max() > 0
    assert g_got["0.module.rnns.1." + rnn_w.rsplit(".", 1)[1]].abs().max() > 0


def test_frozen_encoder_runs_every_chunk_without_grad():
    model = tiny()
    ClassifierTrainer(model).freeze()
    ids = torch.randint(2, 50, (3, 20))
    hidden, lens = model[0](ids, torch.tensor([20, 7, 1]))
    assert not hidden.requires_grad and hidden.shape == (3, 20, 16)
    assert lens.tolist() == [20, 7, 1]


def test_cpu_pool_window_matches_explicit_slices():
    torch.manual_seed(0)
    h = torch.randn(4, 9, 6)
    lens = torch.tensor([9, 1, 5, 12])          # 12 clamps to T
    for max_len in (1, 3, 20):
        got = _cpu_concat_pool(h, lens, max_len)
        for b, l in enumerate([9, 1, 5, 9]):
            w = h[b, max(0, l - max_len):l]
            want = torch.cat([w.mean(0), w.max(0).values, w[-1]])
            assert torch.allclose(got[b], want, atol=1e-6)
    # a window wider than every row is the unwindowed pool
    base = _cpu_concat_pool(h[:3], lens[:3])
    assert torch.allclose(base, _cpu_concat_pool(h[:3], lens[:3], 20), atol=1e-6)


# --- training ---------------------------------------------------------------

def test_tiny_fit_halves_bce():
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(2)
    docs = [torch.randint(2, 50, (int(n),), generator=g).tolist()
            for n in torch.randint(6, 13, (8,), generator=g)]
    y = (torch.rand(8, 3, generator=g) < 0.5).float()
    model = tiny(bptt=8, max_len=10)
    tr = ClassifierTrainer(model, multi_label=True, wd=0.0)
    tr.unfreeze()
    loader = PaddedBatchLoader(docs, y, bs=8, pad_token=1, shuffle=False)
    losses = tr.fit(loader, epochs=200, lr=1e-2)
    assert len(losses) == 200
    assert all(math.isfinite(l) for l in losses)
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
    m = tr.evaluate(loader)
    assert 0.0 <= m["accuracy"] <= 1.0 and math.isfinite(m["valid_loss"])


def test_one_cycle_scales_each_group_and_save_load(tmp_path):
    torch.manual_seed(0)
    model = tiny()
    tr = ClassifierTrainer(model, multi_label=False)
    docs = [[5, 6, 7, 8], [9, 10], [11, 12, 13], [14]]
    loader = PaddedBatchLoader(docs, [0, 1, 2, 1], bs=2, shuffle=False)
    batches = list(loader)
    assert [b[0].shape for b in batches] == [(2, 4), (2, 2)]
    assert batches[0][1].tolist() == [4, 3] and batches[1][0][1].tolist() == [14, 1]
    tr.freeze_to(-2)
    tr.fit_one_cycle(loader, epochs=2, max_lr=slice(1e-3))
    lrs = [g["lr"] for g in tr.opt.param_groups]
    assert lrs[-1] == pytest.approx(10 * lrs[0]) and 0 < lrs[-1] < 1e-3
    assert tr.evaluate(loader)["accuracy"] <= 1.0
    tr.save(tmp_path / "clas.pth")
    other = ClassifierTrainer(tiny(), multi_label=False)
    other.load(tmp_path / "clas.pth")
    for (n, a), (_, b) in zip(model.state_dict().items(),
                              other.model.state_dict().items()):
        assert torch.equal(a, b), n
    assert other.global_step == tr.global_step == 4


def test_finetune_cli_runs_notebook_schedule(tmp_path):
    from code_intelligence_amd.engine.inference import save_artifacts
    from code_intelligence_amd.text.tokenizer import Tokenizer, Vocab
    from code_intelligence_amd.train import finetune_cli
    texts = [f"crash in module{i % 3} when saving file number {i}"
             for i in range(12)]
    vocab = Vocab.create(Tokenizer().process_all(texts), min_freq=1)
    torch.manual_seed(0)
    lm = AWDLSTM(vocab_sz=len(vocab), emb_sz=8, n_hid=12, n_layers=2)
    save_artifacts(lm, vocab, tmp_path / "lm")
    rows = [{"text": t, "labels": ["bug"] + (["io"] if i % 2 else [])}
            for i, t in enumerate(texts)]
    (tmp_path / "d.jsonl").write_text("\n".join(json.dumps(r) for r in rows))
    out = finetune_cli.main([
        "--artifacts", str(tmp_path / "lm"), "--data", str(tmp_path / "d.jsonl"),
        "--out", str(tmp_path / "clas.pth"), "--bs", "4", "--bptt", "5",
        "--device", "cpu", "--valid_pct", "0.25"])
    assert out["labels"] == 2 and math.isfinite(out["final"]["valid_loss"])
    assert (tmp_path / "clas.pth").exists()
    assert json.loads((tmp_path / "clas.pth.labels.json").read_text()) == ["bug", "io"]
