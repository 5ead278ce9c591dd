"""InferenceWrapper — the embedding inference engine (serve hot path).

API-compatible re-creation of py/code_intelligence/inference.py:25-263:
``process_dict``, ``get_pooled_features`` (-> (1, 3*emb_sz) = 2400-d at the
deployed config), ``df_to_embedding`` (sort-by-length batching, padding,
OOM backoff halving bs — inference.py:138-229), ``batch_seq_pool``
(length-masked pooling, inference.py:232-263 — here the K5 HIP kernel).

MI355X design: the encoder runs the fused CDNA4 LSTM kernels; fixed-length
buckets can be hipGraph-captured (engine/graph_exec.py) to kill the
per-timestep launch overhead that dominates at serve batch sizes.
"""
from __future__ import annotations

import json
import logging
import os
import threading
from pathlib import Path
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from ..models.awd_lstm import AWDLSTM, AWDLSTMEncoder, LinearDecoder
from ..ops.pool import concat_pool
from ..text.tokenizer import (BOS, UNK, Tokenizer, Vocab, decode_spec_tokens,
                              process_dict as _process_dict)

log = logging.getLogger(__name__)


class InferenceWrapper:
    """Loads model artifacts and turns (title, body) into pooled embeddings."""

    def __init__(self, model_path: Optional[str] = None,
                 model_file_name: Optional[str] = None,
                 encoder: Optional[AWDLSTMEncoder] = None,
                 vocab: Optional[Vocab] = None,
                 device: Optional[str] = None,
                 dtype: Optional[torch.dtype] = None,
                 use_graphs: bool = False,
                 decoder: Optional[LinearDecoder] = None):
        self.device = torch.device(device) if device else (
            torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
        self.dtype = dtype or (torch.bfloat16 if self.device.type == "cuda"
                               else torch.float32)
        self.tokenizer = Tokenizer()
        if encoder is not None:
            assert vocab is not None
            self.encoder, self.vocab = encoder, vocab
            self.decoder = decoder
        else:
            root = Path(model_path)
            if model_file_name:
                root = root / model_file_name
            cfg = json.loads((root / "config.json").read_text())
            self.vocab = Vocab.load(root / "vocab.json")
            dec_sd = None
            if cfg.get("decoder_file"):
                dec_sd = torch.load(root / cfg["decoder_file"],
                                    map_location="cpu", weights_only=True)
            model = AWDLSTM(vocab_sz=len(self.vocab), emb_sz=cfg["emb_sz"],
                            n_hid=cfg["n_hid"], n_layers=cfg["n_layers"],
                            qrnn=cfg.get("qrnn", False),
                            tie_weights=cfg.get("tie_weights", True),
                            out_bias=dec_sd is None or "bias" in dec_sd)
            enc_file = root / cfg.get("encoder_file", "encoder.pth")
            model.load_encoder(enc_file)
            self.encoder = model.encoder
            self.decoder = decoder
            if dec_sd is not None and decoder is None:
                # strict=False: a tied weight lives in encoder.pth only
                model.decoder.decoder.load_state_dict(dec_sd, strict=False)
                self.decoder = model.decoder
        self.encoder = self.encoder.to(device=self.device, dtype=self.dtype)
        self.encoder.eval()
        self._lm: Optional[AWDLSTM] = None
        if self.decoder is not None:
            # moving the encoder first keeps a tied weight one Parameter
            self.decoder = self.decoder.to(device=self.device, dtype=self.dtype)
            self.decoder.eval()
            self._lm = AWDLSTM.from_parts(self.encoder, self.decoder)
        self.emb_sz = self.encoder.emb_sz
        self.pad_idx = self.encoder.pad_token
        self._graphs = {}
        # the encoder carries hidden state across forward calls; serialize
        # encodes so a threaded caller gets correct (serialized) results
        # instead of silently corrupted ones (reference serving is
        # single-threaded, app.py:128 — this guards misuse)
        self._encode_lock = threading.Lock()
        self.use_graphs = use_graphs and self.device.type == "cuda"
        # (r1 gated QRNN graphs off after replay memory-faults; diagnosed
        # in r2 as WeightDroppedQRNN reassigning prev_x to a capture-pool
        # allocation — fixed by copying into a stable buffer, validated by
        # scripts/qrnn_graph_repro.py rung 7. Graphs remain opt-in for
        # both encoder families: bucket padding outweighs launch savings
        # at measured shapes, profiles/BENCH_HISTORY.md.)

    # --- reference-parity helpers -----------------------------------------
    def process_dict(self, data: dict) -> dict:
        return _process_dict(data, self.tokenizer)

    def numericalize(self, text: str) -> List[int]:
        ids = self.vocab.numericalize(self.tokenizer.process_text(text))
        # serve-side length cap (CI_SERVE_MAX_TOKENS=N, 0 = unlimited): a
        # pathological multi-MB issue body otherwise runs unbounded
        # recurrent timesteps on a single-threaded server. Default 10000
        # tokens (~40 KB of text) — far beyond any real issue; the
        # reference survived the same exposure only by having 9 replicas.
        cap = int(os.environ.get("CI_SERVE_MAX_TOKENS", "10000"))
        return ids[:cap] if cap > 0 else ids

    @staticmethod
    def _bucket(n: int, buckets=(1, 2, 4, 8, 16, 24, 32, 48, 64, 96, 128,
                                 192, 256, 384, 512, 768, 1024, 1536, 2048)) -> int:
        # ~1.5x-spaced buckets: worst-case padding 50%, typical ~20%
        for b in buckets:
            if n <= b:
                return b
        return n

    @torch.no_grad()
    def _encode_batch(self, ids: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """ids: (B, T) padded; returns (B, 3*emb_sz) pooled fp32."""
        with self._encode_lock:
            return self._encode_batch_locked(ids, lengths)

    def _encode_batch_locked(self, ids: torch.Tensor, lengths: torch.Tensor
                             ) -> torch.Tensor:
        B, T = ids.shape
        if self.use_graphs:
            # pad (B, T) up to fixed buckets so each shape is captured once
            Bb, Tb = self._bucket(B), self._bucket(T)
            if (Bb, Tb) != (B, T):
                padded = torch.full((Bb, Tb), self.pad_idx, dtype=ids.dtype,
                                    device=ids.device)
                padded[:B, :T] = ids
                ids = padded
            from .graph_exec import GraphedEncoder
            key = (Bb, Tb)
            if key not in self._graphs:
                self._graphs[key] = GraphedEncoder(self.encoder, Bb, Tb, self.device)
            hidden = self._graphs[key].run(ids)[:B]
        else:
            self.encoder.reset(B)
            _, outputs = self.encoder(ids)
            hidden = outputs[-1]
        return concat_pool(hidden, lengths).float()

    @torch.no_grad()
    def get_pooled_features(self, text: str) -> torch.Tensor:
        """(1, 3*emb_sz) embedding for one document (inference.py:74-93)."""
        ids = self.numericalize(text)
        if not ids:
            ids = [self.vocab.stoi.get("xxunk", 0)]
        t = torch.tensor([ids], dtype=torch.int64, device=self.device)
        lens = torch.tensor([len(ids)], device=self.device)
        return self._encode_batch(t, lens).cpu()

    def predict(self, text: str, n_words: int = 1, no_unk: bool = True,
                temperature: float = 1.0, min_p: Optional[float] = None,
                sep: str = " ", seed: Optional[int] = None,
                n_samples: int = 1, top_k: Optional[int] = None,
                top_p: Optional[float] = None) -> Union[str, List[str]]:
        """Continue ``text`` by ``n_words`` sampled tokens — fastai
        ``LanguageLearner.predict`` (the reference's post-pretraining check,
        04_Inference.ipynb). Returns ``text + sep + continuation``; with
        ``n_samples > 1`` a list of that many continuations of the same
        prompt, each drawn with its own stream of uniforms. ``top_k`` /
        ``top_p`` restrict every draw to the k most likely words / the
        smallest set of words that holds ``top_p`` of the probability
        (``AWDLSTM.generate``); ``None`` is no filter."""
        if self._lm is None:
            raise RuntimeError(
                "this artifact has no decoder, so it cannot generate text: "
                "export it with save_artifacts(..., with_decoder=True)")
        if n_samples < 1:
            raise ValueError(f"n_samples must be >= 1 (got {n_samples})")
        stoi = self.vocab.stoi
        unk = stoi.get(UNK, 0)
        ids = self.numericalize(text) or [stoi.get(BOS, unk)]
        prompt = torch.tensor([ids] * n_samples, dtype=torch.int64,
                              device=self.device)
        with self._encode_lock:
            out, _ = self._lm.generate(prompt, n_words, temperature=temperature,
                                       min_p=min_p, no_unk=no_unk, unk_idx=unk,
                                       seed=seed, top_k=top_k, top_p=top_p)
        texts = [text + sep + sep.join(decode_spec_tokens(
            self.vocab.itos[i] for i in row)) for row in out.cpu().tolist()]
        return texts[0] if n_samples == 1 else texts

    def beam_search(self, text: str, n_words: int, no_unk: bool = True,
                    top_k: int = 10, beam_sz: int = 1000,
                    temperature: float = 1.0, sep: str = " ",
                    decoder=decode_spec_tokens,
                    seed: Optional[int] = None) -> str:
        """Continue ``text`` by ``n_words`` tokens found by beam search —
        fastai ``LanguageLearner.beam_search``: every word keeps the
        ``beam_sz`` best of each beam's ``top_k`` continuations, and one of
        the final beams is drawn with probability proportional to
        ``exp(-score / temperature)``. Returns ``text + sep + continuation``;
        deterministic for a given ``seed``."""
        if self._lm is None:
            raise RuntimeError(
                "this artifact has no decoder, so it cannot generate text: "
                "export it with save_artifacts(..., with_decoder=True)")
        stoi = self.vocab.stoi
        unk = stoi.get(UNK, 0)
        ids = self.numericalize(text) or [stoi.get(BOS, unk)]
        prompt = torch.tensor([ids], dtype=torch.int64, device=self.device)
        with self._encode_lock:
            out, _, _ = self._lm.beam_search(
                prompt, n_words, top_k=top_k, beam_sz=beam_sz, no_unk=no_unk,
                unk_idx=unk, temperature=temperature, seed=seed)
        return text + sep + sep.join(decoder(
            self.vocab.itos[i] for i in out.tolist()))

    def df_to_embedding(self, dataframe, bs: int = 100) -> np.ndarray:
        """Bulk path (inference.py:138-229): build docs from (title, body)
        rows, sort by length, pad per batch, encode, unsort. OOM -> bs//2."""
        texts = [self.process_dict({"title": t, "body": b})["text"]
                 for t, b in zip(dataframe["title"], dataframe["body"])]
        return self.texts_to_embedding(texts, bs=bs)

    def texts_to_embedding(self, texts: Sequence[str], bs: int = 100) -> np.ndarray:
        # batched tokenization (native GIL-released core underneath)
        cap = int(os.environ.get("CI_SERVE_MAX_TOKENS", "10000"))
        tok_lists = self.tokenizer.process_all(list(texts))
        docs = []
        for toks in tok_lists:
            ids = self.vocab.numericalize(toks)
            if cap > 0:
                ids = ids[:cap]
            docs.append(ids or [0])
        order = sorted(range(len(docs)), key=lambda i: len(docs[i]))
        out = np.empty((len(docs), 3 * self.emb_sz), dtype=np.float32)
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
                    pooled = self._encode_batch(ids.to(self.device),
                                                lens.to(self.device))
                    break
                except torch.cuda.OutOfMemoryError:
                    # reference behavior: halve the batch until it fits
                    # (inference.py:214-223)
                    torch.cuda.empty_cache()
                    cur_bs //= 2
                    if cur_bs < 1:
                        raise
            pooled_np = pooled.cpu().numpy()  # one D2H copy per batch
            for r, j in enumerate(idxs):
                out[j] = pooled_np[r]
            i += len(idxs)
        return out

    # alias matching the flask-app copy (Issue_Embeddings/flask_app/inference.py)
    df_to_emb = df_to_embedding

    def batch_seq_pool(self, hidden: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        return concat_pool(hidden, lengths)


def save_artifacts(model: AWDLSTM, vocab: Vocab, path,
                   with_decoder: bool = False) -> None:
    """Write the artifact layout InferenceWrapper loads. ``with_decoder``
    adds ``decoder.pth`` (the output bias, and the weight when it is not tied
    to the embedding) so the served model can ``predict`` text."""
    root = Path(path)
    root.mkdir(parents=True, exist_ok=True)
    enc = model.encoder
    cfg = {
        "emb_sz": enc.emb_sz, "n_hid": enc.n_hid, "n_layers": enc.n_layers,
        "qrnn": bool(getattr(enc, "qrnn", False)),
        "encoder_file": "encoder.pth"}
    if with_decoder:
        lin = model.decoder.decoder
        tied = lin.weight is enc.encoder.weight
        cfg["decoder_file"] = "decoder.pth"
        cfg["tie_weights"] = tied
        torch.save({k: v for k, v in lin.state_dict().items()
                    if not (tied and k == "weight")}, root / "decoder.pth")
    (root / "config.json").write_text(json.dumps(cfg))
    vocab.save(root / "vocab.json")
    model.save_encoder(root / "encoder.pth")
