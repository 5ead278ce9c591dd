"""End-to-end classifier fine-tuning with gradual unfreezing (reference:
Issue_Embeddings/notebooks/06_FineTune.ipynb — ``freeze(); fit_one_cycle``,
then ``freeze_to(-2)`` and training through the LSTM layers with
discriminative learning rates ``lr=slice(...)``).

Unlike train/transfer.py (frozen pooled features -> MLP) the loss here
backpropagates through the concat-pool kernel pair into the encoder's own
LSTM/QRNN backward kernels. Layer groups follow fastai's
``awd_lstm_clas_split``; each is one FusedAdamW param group so a step takes
one learning rate per group."""
from __future__ import annotations

from typing import Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from ..models.classifier import TextClassifier
from ..ops.adam import FusedAdamW
from ..parallel.ddp import DistributedGrads, broadcast_parameters
from .schedules import OneCycle

__all__ = ["ClassifierTrainer", "PaddedBatchLoader"]

LR = Union[float, slice]


class PaddedBatchLoader:
    """Sort-by-length padded batches over ``(ids list, label vector)`` pairs.

    Documents are sorted by length (longest first, so the largest batch
    comes first and an out-of-memory shows at once), cut into batches, and
    END-padded with ``pad_token``; the batch order is shuffled each epoch
    when ``shuffle``; ``drop_last`` drops an incomplete final batch (fastai's
    training loaders do). Yields ``(ids (B,T) int64, lengths (B,) int64,
    labels (B,C) float32 | (B,) int64)``."""

    def __init__(self, docs: Sequence[Sequence[int]], labels: Sequence,
                 bs: int = 32, pad_token: int = 1, device="cpu",
                 shuffle: bool = True, seed: int = 0,
                 drop_last: bool = False):
        if len(docs) != len(labels):
            raise ValueError("docs and labels differ in length")
        self.docs, self.bs, self.pad_token = docs, bs, pad_token
        self.labels = torch.as_tensor(labels)
        if self.labels.is_floating_point() or self.labels.dim() == 2:
            self.labels = self.labels.float()
        self.device, self.shuffle = device, shuffle
        self._gen = torch.Generator().manual_seed(seed)
        order = sorted(range(len(docs)), key=lambda i: -len(docs[i]))
        self.batches = [order[i:i + bs] for i in range(0, len(order), bs)]
        if drop_last and len(self.batches) > 1 and len(self.batches[-1]) < bs:
            self.batches.pop()  # training: BatchNorm cannot take a batch of 1

    def __len__(self) -> int:
        return len(self.batches)

    def __iter__(self) -> Iterator[Tuple[Tensor, Tensor, Tensor]]:
        idx = torch.randperm(len(self.batches), generator=self._gen).tolist() \
            if self.shuffle else range(len(self.batches))
        for bi in idx:
            rows = self.batches[bi]
            lens = torch.tensor([max(1, len(self.docs[i])) for i in rows])
            ids = torch.full((len(rows), int(lens.max())), self.pad_token,
                             dtype=torch.long)
            for r, i in enumerate(rows):
                d = self.docs[i]
                ids[r, :len(d)] = torch.as_tensor(d, dtype=torch.long)
            yield (ids.to(self.device), lens.to(self.device),
                   self.labels[rows].to(self.device))


class ClassifierTrainer:
    def __init__(self, model: TextClassifier, multi_label: bool = True,
                 wd: float = 0.01, distributed: bool = False,
                 threshold: float = 0.5):
        self.model = model
        self.multi_label, self.threshold = multi_label, threshold
        enc = model.encoder
        # fastai awd_lstm_clas_split: [embedding], one per rnn, [head]
        self.groups: List[List[nn.Module]] = \
            [[enc.encoder, enc.encoder_dp]] + \
            [[rnn, dp] for rnn, dp in zip(enc.rnns, enc.hidden_dps)] + \
            [[model.head]]
        self.opt = FusedAdamW(
            [{"params": self._group_params(g)} for g in self.groups],
            weight_decay=wd)
        self.lossf = nn.BCEWithLogitsLoss() if multi_label \
            else nn.CrossEntropyLoss()
        self.global_step = 0
        if distributed:
            # built while every parameter is trainable: groups frozen later
            # simply bring no grad, which finalize() zero-fills
            broadcast_parameters(model)
            self.dist: Optional[DistributedGrads] = DistributedGrads(model)
        else:
            self.dist = None

    # --- layer groups ------------------------------------------------------
    @staticmethod
    def _group_params(mods: Iterable[nn.Module]) -> List[nn.Parameter]:
        seen, out = set(), []
        for m in mods:
            for p in m.parameters():
                if id(p) not in seen:  # encoder_dp.emb is the embedding
                    seen.add(id(p))
                    out.append(p)
        return out

    def freeze_to(self, n: int) -> None:
        """Freeze ``groups[:n]``, make ``groups[n:]`` trainable."""
        frozen = set(range(len(self.groups))[:n])
        for i, g in enumerate(self.groups):
            for p in self._group_params(g):
                p.requires_grad_(i not in frozen)

    def freeze(self) -> None:
        self.freeze_to(-1)

    def unfreeze(self) -> None:
        self.freeze_to(0)

    def lr_range(self, lr: LR) -> List[float]:
        """fastai semantics: a float for every group; ``slice(stop)`` gives
        the last group ``stop`` and the others ``stop/10``;
        ``slice(start, stop)`` spaces the groups geometrically."""
        n = len(self.groups)
        if not isinstance(lr, slice):
            return [float(lr)] * n
        if lr.start is None:
            return [lr.stop / 10.0] * (n - 1) + [float(lr.stop)]
        if n == 1:
            return [float(lr.stop)]
        ratio = lr.stop / lr.start
        return [lr.start * ratio ** (i / (n - 1)) for i in range(n)]

    # --- training ----------------------------------------------------------
    def _loss(self, logits: Tensor, y: Tensor) -> Tensor:
        if self.multi_label:
            return self.lossf(logits, y.to(logits.dtype))
        return self.lossf(logits, y.long())

    def train_step(self, ids: Tensor, lengths: Tensor, y: Tensor,
                   lrs: Union[float, Sequence[float]],
                   mom: Optional[float] = None) -> float:
        if isinstance(lrs, (int, float)):
            lrs = [float(lrs)] * len(self.groups)
        for g, lr in zip(self.opt.param_groups, lrs):
            g["lr"] = lr
            if mom is not None:
                g["betas"] = (mom, g["betas"][1])
        self.opt.zero_grad(set_to_none=True)
        if self.dist is not None:
            self.dist.prepare()
        loss = self._loss(self.model(ids, lengths), y)
        loss.backward()
        if ids.is_cuda:
            from ..ops.lstm import sync_dw_stream
            sync_dw_stream()
        if self.dist is not None:
            self.dist.finalize()
        self.opt.step()
        self.global_step += 1
        return float(loss.detach())

    def _run(self, loader, epochs: int, lrs: List[float],
             sched: Optional[OneCycle]) -> List[float]:
        self.model.train()
        total = max(1, epochs * len(loader))
        losses, step = [], 0
        for _ in range(epochs):
            for ids, lengths, y in loader:
                scale, mom = sched.at(step / total) if sched else (1.0, None)
                losses.append(self.train_step(
                    ids, lengths, y, [lr * scale for lr in lrs], mom))
                step += 1
        return losses

    def fit_one_cycle(self, loader, epochs: int, max_lr: LR) -> List[float]:
        """One-cycle over ``epochs``; the cycle's shape (train/schedules.py,
        peak 1.0) scales every group's own maximum."""
        return self._run(loader, epochs, self.lr_range(max_lr),
                         OneCycle(max_lr=1.0))

    def fit(self, loader, epochs: int, lr: LR) -> List[float]:
        return self._run(loader, epochs, self.lr_range(lr), None)

    @torch.no_grad()
    def evaluate(self, loader) -> dict:
        """Mean loss and accuracy: thresholded per-label accuracy when
        ``multi_label`` (fastai ``accuracy_thresh``), else top-1."""
        was_training = self.model.training
        self.model.eval()
        tot, n, correct, cells = 0.0, 0, 0.0, 0
        for ids, lengths, y in loader:
            logits = self.model(ids, lengths)
            tot += float(self._loss(logits, y)) * ids.size(0)
            n += ids.size(0)
            if self.multi_label:
                pred = torch.sigmoid(logits) > self.threshold
                correct += float((pred == (y > 0.5)).sum())
                cells += y.numel()
            else:
                correct += float((logits.argmax(1) == y).sum())
                cells += ids.size(0)
        self.model.train(was_training)
        return {"valid_loss": tot / max(n, 1),
                "accuracy": correct / max(cells, 1)}

    # --- checkpoint --------------------------------------------------------
    def save(self, path) -> None:
        torch.save({"model": self.model.state_dict(),
                    "optimizer": self.opt.state_dict(),
                    "global_step": self.global_step}, path)

    def load(self, path, map_location="cpu") -> None:
        ckpt = torch.load(path, map_location=map_location, weights_only=False)
        self.model.load_state_dict(ckpt["model"])
        self.opt.load_state_dict(ckpt["optimizer"])
        self.global_step = ckpt.get("global_step", 0)
