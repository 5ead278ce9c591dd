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

import weakref
from itertools import chain
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from ..ops.pool import (StreamingConcatPool, concat_pool, head_fits_lds,
                        pool_head)
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
        self.max_live_chunks = 0  # most chunks seen alive at once, last stream_pool

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

    @torch.no_grad()
    def stream_pool(self, ids: Tensor, lengths: Tensor,
                    dtype: torch.dtype = torch.float32) -> StreamingConcatPool:
        """Inference-only walk: the chunks, reset, length clamp and skipped
        prefix of ``forward``, but every chunk is folded into a
        ``StreamingConcatPool`` and dropped before the next encoder call, so
        one chunk of hidden states is alive at a time whatever the document
        length. ``max_live_chunks`` records what was observed: 1 plus whether
        the previous chunk's final-layer tensor was still referenced when an
        encoder call started. Returns the pool (absolute lengths, ``max_len``
        window)."""
        B, T = ids.shape
        lens = lengths.to(ids.device).clamp(1, T)
        g = int((lens - self.max_len).clamp_min(0).min())
        self.module.reset(B)
        pool = StreamingConcatPool(B, self.module.emb_sz, self.max_len,
                                   ids.device, dtype)
        lens_p = lens.to(torch.int32) if ids.is_cuda else lens
        self.max_live_chunks = 0
        prev = None     # weak reference to the previous chunk's final states
        for s in range(0, T, self.bptt):
            e = min(s + self.bptt, T)
            if e <= g:
                self.module(ids[:, s:e])
                continue
            # observed, not assumed: is the previous chunk's tensor still
            # referenced anywhere as the next encoder call starts?
            carried = int(prev is not None and prev() is not None)
            # bind the final layer's states only: the encoder's two per-layer
            # lists die with this expression
            h = self.module(ids[:, s:e])[1][-1]
            self.max_live_chunks = max(self.max_live_chunks, carried + 1)
            pool.update(h, lens_p, s)
            prev = weakref.ref(h)
            del h
        return pool


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


@torch.no_grad()
def fold_head_bn(head: PoolingLinearClassifier
                 ) -> Optional[Tuple[Tensor, Tensor, Tensor, Tensor]]:
    """Fold the eval-mode BatchNorms of the standard head into its Linears.

    Accepts exactly ``BatchNorm1d, Dropout, Linear, ReLU, BatchNorm1d,
    Dropout, Linear`` (``None`` for anything else). With s = gamma /
    sqrt(var + eps) and t = beta - mean * s, ``Linear(BN(x))`` is
    ``(W * s) x + (W t + b)``; the fold runs in fp64 and is rounded to fp32
    once. Returns ``(w1, b1, w2, b2)``."""
    mods = list(head.layers)
    kinds = (nn.BatchNorm1d, nn.Dropout, nn.Linear, nn.ReLU,
             nn.BatchNorm1d, nn.Dropout, nn.Linear)
    if len(mods) != len(kinds) or not all(
            type(m) is k for m, k in zip(mods, kinds)):
        return None
    out: List[Tensor] = []
    for bn, lin in ((mods[0], mods[2]), (mods[4], mods[6])):
        if bn.running_mean is None or bn.running_var is None:
            return None
        s = (bn.running_var.double() + bn.eps).rsqrt()
        t = -bn.running_mean.double() * s
        if bn.affine:
            s, t = s * bn.weight.double(), t * bn.weight.double() + bn.bias.double()
        w = lin.weight.double()
        b = w @ t
        if lin.bias is not None:
            b = b + lin.bias.double()
        out += [(w * s).float().contiguous(), b.float().contiguous()]
    return out[0], out[1], out[2], out[3]


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

    # --- inference ---------------------------------------------------------
    _folded: Optional[Tuple[Tensor, Tensor, Tensor, Tensor]] = None
    _fold_tried = False

    def train(self, mode: bool = True):
        if mode:
            self._folded, self._fold_tried = None, False
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self._folded, self._fold_tried = None, False
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._folded, self._fold_tried = None, False
        return super()._apply(fn, *args, **kwargs)

    def _folded_head(self) -> Optional[Tuple[Tensor, Tensor, Tensor, Tensor]]:
        """Cached ``fold_head_bn(self.head)``; dropped by ``train()``,
        ``load_state_dict`` and device/dtype moves. Parameters edited in
        place while the model stays in eval mode are not noticed."""
        if not self._fold_tried:
            self._folded, self._fold_tried = fold_head_bn(self.head), True
        return self._folded

    def predict_proba(self, ids: Tensor, lengths: Tensor,
                      multi_label: bool = True) -> Tuple[Tensor, Tensor]:
        """ids (B,T) end-padded, lengths (B,) -> (probs, logits), fp32 (B, C).

        Every module is put in eval mode and ``no_grad`` holds for the call;
        afterwards each module gets its own training flag back (frozen groups
        that were in eval under a training root stay in eval). The document
        is streamed through ``stream_pool``; the standard one-hidden-layer
        head then runs BatchNorm-folded in one fused launch, any other head
        as ``self.head`` on the streamed features."""
        flags = [(m, m.training) for m in self.modules()]
        if any(f for _, f in flags):
            # something was training: its weights or BatchNorm statistics
            # may have moved since the head was last folded
            self._folded, self._fold_tried = None, False
            for m, _ in flags:
                m.training = False
        try:
            with torch.no_grad():
                pool = self[0].stream_pool(ids, lengths)
                folded = self._folded_head()
                if folded is not None and head_fits_lds(
                        pool.H, folded[0].size(0), folded[2].size(0)):
                    return pool_head(pool.state, pool.lengths, pool.max_len,
                                     *folded, multi_label=multi_label)
                logits = self[1](pool.features().float())
                probs = torch.sigmoid(logits) if multi_label \
                    else torch.softmax(logits, dim=1)
                return probs, logits
        finally:
            for m, f in flags:
                m.training = f

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
