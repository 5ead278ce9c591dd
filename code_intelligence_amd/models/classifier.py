"""ULMFiT text classifier: pretrained AWD-LSTM/QRNN encoder + pooling head.

Re-creates the model that the reference's last pipeline stage fine-tunes
(Issue_Embeddings/notebooks/06_FineTune.ipynb: ``text_classifier_learner``
on the LM config minus ``tie_weights``/``out_bias``, ``load_encoder``, then
gradual unfreezing through the LSTM layers).

Structure follows fastai's ``SequentialRNN(MultiBatchEncoder(AWD_LSTM),
PoolingLinearClassifier)``, so state-dict keys are ``0.module.<encoder key>``
and ``1.layers.{0,2,4,6}.*`` and ``save_encoder`` artifacts load into
``model[0].module``. Two deliberate differences:

* The pooled feature order stays this project's ``[mean, max, last]`` (the
  serve path's concat-pool); fastai concatenates ``[last, max, mean]``. The
  first head layers therefore see permuted inputs and fastai *classifier*
  checkpoints are NOT importable (encoder checkpoints are).
* Batches are end-padded (this project's loaders), so "keep the last
  ``max_len`` positions" is a per-row window ``[len_b - max_len, len_b)``
  applied inside the pool kernel rather than a slice of a front-padded batch.
"""
from __future__ import annotations

from itertools import chain
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from ..ops.pool import concat_pool
from .awd_lstm import AWDLSTMEncoder

__all__ = [
    "MultiBatchEncoder",
    "PoolingLinearClassifier",
    "TextClassifier",
    "get_text_classifier",
    "awd_lstm_clas_config",
]

# This project's classifier defaults: the LM architecture with heavier
# dropout for the small labelled set. fastai is not installed here, so these
# are NOT verified against fastai's awd_lstm_clas_config; the reference
# notebook passes its own (LM) config anyway.
awd_lstm_clas_config = dict(
    emb_sz=400,
    n_hid=1150,
    n_layers=3,
    pad_token=1,
    qrnn=False,
    bidir=False,
    output_p=0.4,
    hidden_p=0.3,
    input_p=0.4,
    embed_p=0.05,
    weight_p=0.5,
)


class MultiBatchEncoder(nn.Module):
    """Feed a long document batch to the encoder in ``bptt``-sized chunks.

    The encoder carries its hidden state from one call to the next and
    detaches it, so gradients flow within a chunk only (fastai's truncated
    BPTT). Chunks that end before every row's pooling window starts
    (``e <= min_b lo_b``) only advance the state: they run under
    ``no_grad`` and their outputs are dropped.

    ``forward`` returns the kept final-layer states as a (B, T', H)
    transpose view of time-major (T', B, H) storage — the LSTM kernels'
    native layout, which the pool kernels read in place — and the lengths
    shifted by the dropped prefix.
    """

    def __init__(self, encoder: AWDLSTMEncoder, bptt: int = 70,
                 max_len: int = 1400):
        super().__init__()
        if bptt < 1 or max_len < 1:
            raise ValueError("bptt and max_len must be >= 1")
        self.module = encoder
        self.bptt, self.max_len = bptt, max_len
        self.kept_chunks = 0  # of the last forward (introspection/tests)

    def reset(self, bs: Optional[int] = None) -> None:
        self.module.reset(bs)

    def forward(self, ids: Tensor, lengths: Tensor) -> Tuple[Tensor, Tensor]:
        B, T = ids.shape
        lens = lengths.to(ids.device).clamp(1, T)
        g = int((lens - self.max_len).clamp_min(0).min())
        self.module.reset(B)
        with_grad = torch.is_grad_enabled() and any(
            p.requires_grad for p in self.module.parameters())
        kept: List[Tensor] = []
        start = 0
        for s in range(0, T, self.bptt):
            e = min(s + self.bptt, T)
            if e <= g:
                with torch.no_grad():
                    self.module(ids[:, s:e])
                continue
            if not kept:
                start = s
            with torch.set_grad_enabled(with_grad):
                _, outputs = self.module(ids[:, s:e])
            kept.append(outputs[-1].transpose(0, 1))      # (T_c, B, H)
        self.kept_chunks = len(kept)
        hidden_tm = kept[0] if len(kept) == 1 else torch.cat(kept, dim=0)
        return hidden_tm.transpose(0, 1), lens - start


class PoolingLinearClassifier(nn.Module):
    """fastai's ``bn_drop_lin`` stack over the concat-pooled features:
    BatchNorm1d -> Dropout -> Linear -> ReLU -> ... -> Linear. The Dropout
    is kept even at p=0 so parameter keys are always ``layers.0/2/4/6.*``.
    Stays in fp32 whatever dtype the model is cast to (BatchNorm statistics
    and the tiny GEMMs gain nothing from bf16)."""

    def __init__(self, layers: Sequence[int], ps: Sequence[float]):
        super().__init__()
        if len(ps) != len(layers) - 1:
            raise ValueError("need one dropout p per linear layer")
        mods: List[nn.Module] = []
        n = len(layers) - 1
        for i, (n_in, n_out, p) in enumerate(zip(layers[:-1], layers[1:], ps)):
            mods += [nn.BatchNorm1d(n_in), nn.Dropout(p), nn.Linear(n_in, n_out)]
            if i != n - 1:
                mods.append(nn.ReLU(inplace=True))
        self.layers = nn.Sequential(*mods)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        for t in chain(self.parameters(), self.buffers()):
            if t.is_floating_point() and t.dtype != torch.float32:
                t.data = t.data.float()
        return self

    def forward(self, pooled: Tensor) -> Tensor:
        return self.layers(pooled)


class TextClassifier(nn.Sequential):
    """``[0]`` MultiBatchEncoder (encoder under ``.module``), ``[1]`` head."""

    def __init__(self, encoder: MultiBatchEncoder,
                 head: PoolingLinearClassifier):
        super().__init__(encoder, head)

    @property
    def encoder(self) -> AWDLSTMEncoder:
        return self[0].module

    @property
    def head(self) -> PoolingLinearClassifier:
        return self[1]

    def reset(self, bs: Optional[int] = None) -> None:
        self[0].reset(bs)

    def forward(self, ids: Tensor, lengths: Tensor) -> Tensor:
        """ids (B,T) end-padded, lengths (B,) -> logits (B, n_class)."""
        hidden, lens = self[0](ids, lengths)
        pooled = concat_pool(hidden, lens, self[0].max_len)
        return self[1](pooled.float())

    def load_encoder(self, path, map_location="cpu") -> None:
        """Load what ``AWDLSTM.save_encoder`` / fastai ``save_encoder`` wrote."""
        sd = torch.load(path, map_location=map_location, weights_only=True)
        if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict):
            sd = sd["model"]  # fastai learner .pth wraps under 'model'
        self.encoder.load_state_dict(sd)


def get_text_classifier(vocab_sz: int, n_class: int, bptt: int = 70,
                        max_len: int = 1400, config: Optional[dict] = None,
                        lin_ftrs: Sequence[int] = (50,),
                        ps: Sequence[float] = (0.1,)) -> TextClassifier:
    """Build the classifier like fastai's ``get_text_classifier``.

    ``config`` defaults to ``awd_lstm_clas_config`` — this project's
    defaults (output_p .4, hidden_p .3, input_p .4, embed_p .05, weight_p
    .5), not verified fastai values. An LM config works too: ``tie_weights``
    and ``out_bias`` are ignored, so the notebook's "LM config minus those
    two keys" and the unmodified LM config both build the same model.
    Head widths are ``[3*emb_sz] + lin_ftrs + [n_class]`` with dropouts
    ``[output_p] + ps``.
    """
    cfg = dict(awd_lstm_clas_config if config is None else config)
    cfg.pop("tie_weights", None)
    cfg.pop("out_bias", None)
    if cfg.pop("bidir", False):
        raise NotImplementedError("bidir=True is not supported")
    output_p = cfg.pop("output_p", 0.4)
    encoder = AWDLSTMEncoder(vocab_sz, **cfg)
    head = PoolingLinearClassifier(
        [3 * encoder.emb_sz] + list(lin_ftrs) + [n_class],
        [output_p] + list(ps))
    return TextClassifier(MultiBatchEncoder(encoder, bptt, max_len), head)
