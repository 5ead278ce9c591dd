"""Fine-tuned classifier label model.

Where ``RepoSpecificLabelModel`` posts (title, body) to the embedding server
and runs an MLP on the returned vector, this model owns the whole network: a
``TextClassifier`` fine-tuned through the encoder (``train/finetune_cli.py
--export_dir``), served in-process by ``ClassifierInferenceWrapper``. The
document is built from (title, text) exactly as the embedding server builds
it from the repo-specific model's request; per-label probability thresholds
follow repo_specific_model.py (None => never predict)."""
from __future__ import annotations

import logging
from typing import Dict, List, Optional

from ..engine.classifier_inference import (DEFAULT_THRESHOLD,
                                           ClassifierInferenceWrapper)
from .models import IssueLabelModel

log = logging.getLogger(__name__)


class FineTunedClassifierLabelModel(IssueLabelModel):
    def __init__(self, wrapper: ClassifierInferenceWrapper,
                 thresholds: Optional[Dict[str, Optional[float]]] = None):
        self.wrapper = wrapper
        # per-label dict; a missing label defaults to 0.5, None = never
        self.thresholds = dict(wrapper.thresholds if thresholds is None
                               else thresholds)

    @classmethod
    def from_path(cls, path, device: Optional[str] = None, dtype=None,
                  thresholds: Optional[Dict[str, Optional[float]]] = None
                  ) -> "FineTunedClassifierLabelModel":
        return cls(ClassifierInferenceWrapper(path, device=device, dtype=dtype),
                   thresholds)

    def build_document(self, title: str, text: List[str]) -> str:
        """What serve/app.py's POST /text makes of the repo-specific model's
        {"title": title, "body": "\\n".join(text)} request."""
        return self.wrapper.process_dict(
            {"title": title, "body": "\n".join(text or [])})["text"]

    def predict_issue_labels(self, org: str, repo: str, title: str,
                             text: List[str], context: Optional[dict] = None
                             ) -> Dict[str, float]:
        probs = self.wrapper.predict(self.build_document(title, text))[2]
        out: Dict[str, float] = {}
        for name, p in zip(self.wrapper.labels, probs):
            thr = self.thresholds.get(name, DEFAULT_THRESHOLD)
            if thr is None:
                continue  # never predict (no satisfactory P/R point)
            if p >= thr:
                out[name] = float(p)
        return out
