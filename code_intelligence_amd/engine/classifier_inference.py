"""ClassifierInferenceWrapper — serve a fine-tuned ``TextClassifier``.

The counterpart of ``InferenceWrapper`` for the product of
``train/finetune_cli.py``: where the reference's fine-tuning notebooks end in
``learn.predict(text)[2]`` (the per-label probabilities), this loads the
exported artifact and labels text through ``TextClassifier.predict_proba`` —
the encoder's chunks are pooled as they are produced and the head runs
fused, so memory does not grow with the document.

Artifact layout (``save_classifier_artifacts``): ``config.json``,
``vocab.json``, ``labels.json``, optional ``thresholds.json`` and
``classifier.pth`` (the model ``state_dict`` only, ``weights_only`` loadable).
"""
from __future__ import annotations

import json
import logging
import os
import threading
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..models.awd_lstm import awd_lstm_lm_config
from ..models.classifier import TextClassifier, get_text_classifier
from ..text.tokenizer import Tokenizer, Vocab, process_dict as _process_dict

log = logging.getLogger(__name__)

DEFAULT_THRESHOLD = 0.5


def save_classifier_artifacts(model: TextClassifier, vocab: Vocab,
                              labels: Sequence[str], path,
                              multi_label: bool = True,
                              thresholds: Optional[Dict[str, Optional[float]]] = None
                              ) -> None:
    """Write the artifact layout ``ClassifierInferenceWrapper`` loads."""
    root = Path(path)
    root.mkdir(parents=True, exist_ok=True)
    enc = model.encoder
    linears = [m for m in model.head.layers if isinstance(m, torch.nn.Linear)]
    if linears[-1].out_features != len(labels):
        raise ValueError(f"{len(labels)} labels for a head with "
                         f"{linears[-1].out_features} outputs")
    (root / "config.json").write_text(json.dumps({
        "emb_sz": enc.emb_sz, "n_hid": enc.n_hid, "n_layers": enc.n_layers,
        "qrnn": bool(getattr(enc, "qrnn", False)),
        "bptt": model[0].bptt, "max_len": model[0].max_len,
        "lin_ftrs": [l.out_features for l in linears[:-1]],
        "n_class": len(labels), "multi_label": bool(multi_label),
        "classifier_file": "classifier.pth"}))
    vocab.save(root / "vocab.json")
    (root / "labels.json").write_text(json.dumps(list(labels)))
    if thresholds is not None:
        (root / "thresholds.json").write_text(json.dumps(thresholds))
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()},
               root / "classifier.pth")


class ClassifierInferenceWrapper:
    """Loads a classifier artifact (or takes model + vocab + labels) and turns
    text into per-label probabilities."""

    def __init__(self, model_path: Optional[str] = None,
                 model: Optional[TextClassifier] = None,
                 vocab: Optional[Vocab] = None,
                 labels: Optional[Sequence[str]] = None,
                 device: Optional[str] = None,
                 dtype: Optional[torch.dtype] = None,
                 multi_label: Optional[bool] = None,
                 thresholds: Optional[Dict[str, Optional[float]]] = None):
        self.device = torch.device(device) if device else (
            torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
        self.dtype = dtype or (torch.bfloat16 if self.device.type == "cuda"
                               else torch.float32)
        self.tokenizer = Tokenizer()
        if model is not None:
            assert vocab is not None and labels is not None
            self.model, self.vocab, self.labels = model, vocab, list(labels)
            self.multi_label = True if multi_label is None else multi_label
            self.thresholds = dict(thresholds or {})
        else:
            root = Path(model_path)
            cfg = json.loads((root / "config.json").read_text())
            self.vocab = Vocab.load(root / "vocab.json")
            self.labels = json.loads((root / "labels.json").read_text())
            thr_file = root / "thresholds.json"
            self.thresholds = dict(thresholds) if thresholds is not None else (
                json.loads(thr_file.read_text()) if thr_file.exists() else {})
            self.multi_label = cfg.get("multi_label", True) \
                if multi_label is None else multi_label
            config = dict(awd_lstm_lm_config)
            config.update(emb_sz=cfg["emb_sz"], n_hid=cfg["n_hid"],
                          n_layers=cfg["n_layers"], qrnn=cfg.get("qrnn", False))
            lin_ftrs = list(cfg.get("lin_ftrs", [50]))
            self.model = get_text_classifier(
                len(self.vocab), cfg["n_class"], bptt=cfg["bptt"],
                max_len=cfg["max_len"], config=config, lin_ftrs=lin_ftrs,
                ps=[0.1] * len(lin_ftrs))
            sd = torch.load(root / cfg.get("classifier_file", "classifier.pth"),
                            map_location="cpu", weights_only=True)
            self.model.load_state_dict(sd)
        if len(self.labels) != self._n_class():
            raise ValueError("label list does not match the head's outputs")
        self.model = self.model.to(device=self.device, dtype=self.dtype)
        self.model.eval()
        self.pad_idx = self.model.encoder.pad_token
        # the encoder carries hidden state across calls: serialize encodes
        # (see InferenceWrapper)
        self._encode_lock = threading.Lock()

    def _n_class(self) -> int:
        return [m for m in self.model.head.layers
                if isinstance(m, torch.nn.Linear)][-1].out_features

    # --- text -> ids (InferenceWrapper's rules) -----------------------------
    def process_dict(self, data: dict) -> dict:
        return _process_dict(data, self.tokenizer)

    @staticmethod
    def _cap() -> int:
        return int(os.environ.get("CI_SERVE_MAX_TOKENS", "10000"))

    def numericalize(self, text: str) -> List[int]:
        ids = self.vocab.numericalize(self.tokenizer.process_text(text))
        cap = self._cap()
        ids = ids[:cap] if cap > 0 else ids
        return ids or [self.vocab.stoi.get("xxunk", 0)]

    def threshold(self, label: str) -> Optional[float]:
        """Per-label threshold; a label absent from the dict gets 0.5, an
        explicit ``None`` means the label is never predicted."""
        return self.thresholds.get(label, DEFAULT_THRESHOLD)

    # --- prediction -----------------------------------------------------------
    def _predict_ids(self, ids: torch.Tensor, lengths: torch.Tensor
                     ) -> torch.Tensor:
        with self._encode_lock:
            probs, _ = self.model.predict_proba(ids, lengths, self.multi_label)
        return probs

    def predict(self, text: str) -> Tuple[List[str], np.ndarray, np.ndarray]:
        """fastai's ``learn.predict`` three-tuple: (names of the labels at or
        above their threshold, bool mask (C,), probabilities (C,)). Without
        ``multi_label`` the single arg-max label is named."""
        ids = self.numericalize(text)
        t = torch.tensor([ids], dtype=torch.int64, device=self.device)
        lens = torch.tensor([len(ids)], device=self.device)
        probs = self._predict_ids(t, lens)[0].float().cpu().numpy()
        mask = self._mask(probs)
        return [l for l, m in zip(self.labels, mask) if m], mask, probs

    def _mask(self, probs: np.ndarray) -> np.ndarray:
        if not self.multi_label:
            mask = np.zeros(len(self.labels), dtype=bool)
            mask[int(probs.argmax())] = True
            return mask
        mask = np.zeros(len(self.labels), dtype=bool)
        for i, (label, p) in enumerate(zip(self.labels, probs)):
            thr = self.threshold(label)
            mask[i] = thr is not None and p >= thr
        return mask

    def predict_batch(self, texts: Sequence[str], bs: int = 32) -> np.ndarray:
        """(N, C) probabilities: sort by length, end-pad per batch, predict,
        unsort; an out-of-memory batch is retried at half the size."""
        cap = self._cap()
        unk = self.vocab.stoi.get("xxunk", 0)
        docs = []
        for toks in self.tokenizer.process_all(list(texts)):
            ids = self.vocab.numericalize(toks)
            if cap > 0:
                ids = ids[:cap]
            docs.append(ids or [unk])
        order = sorted(range(len(docs)), key=lambda i: len(docs[i]))
        out = np.empty((len(docs), len(self.labels)), dtype=np.float32)
        i = 0
        while i < len(order):
            cur_bs = bs
            while True:
                idxs = order[i: i + cur_bs]
                batch_docs = [docs[j] for j in idxs]
                T = max(len(d) for d in batch_docs)
                ids = torch.full((len(idxs), T), self.pad_idx, dtype=torch.int64)
                for r, d in enumerate(batch_docs):
                    ids[r, :len(d)] = torch.tensor(d)
                lens = torch.tensor([len(d) for d in batch_docs])
                try:
                    probs = self._predict_ids(ids.to(self.device),
                                              lens.to(self.device))
                    break
                except torch.cuda.OutOfMemoryError:
                    torch.cuda.empty_cache()
                    cur_bs //= 2
                    if cur_bs < 1:
                        raise
            probs_np = probs.float().cpu().numpy()  # one D2H copy per batch
            for r, j in enumerate(idxs):
                out[j] = probs_np[r]
            i += len(idxs)
        return out
