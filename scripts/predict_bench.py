"""Classifier inference latency and peak memory at the fine-tune shape:
``TextClassifier.predict_proba`` (streamed pool + fused head) against the
existing route ``sigmoid(model(ids, lengths))`` under ``no_grad``, on the
deployed 4x2400 encoder (emb 800, vocab 60k), bf16, B=32, T=1400.

The two routes alternate inside one process; each call ends in a device
synchronise. Peak bytes are ``max_memory_allocated`` over one call, given
both as the absolute peak and above what was allocated before the call
(weights and inputs). Informational; prints one JSON line.

Usage: python scripts/predict_bench.py [--bs 32 --seq_len 1400 --rounds 5]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from code_intelligence_amd.models.awd_lstm import awd_lstm_lm_config  # noqa: E402
from code_intelligence_amd.models.classifier import get_text_classifier  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--bs", type=int, default=32)
    p.add_argument("--seq_len", type=int, default=1400)
    p.add_argument("--bptt", type=int, default=70)
    p.add_argument("--max_len", type=int, default=1400)
    p.add_argument("--vocab_sz", type=int, default=60000)
    p.add_argument("--emb_sz", type=int, default=800)
    p.add_argument("--n_hid", type=int, default=2400)
    p.add_argument("--n_layers", type=int, default=4)
    p.add_argument("--n_class", type=int, default=30)
    p.add_argument("--qrnn", action="store_true")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    args = p.parse_args(argv)
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = dict(awd_lstm_lm_config)
    cfg.update(emb_sz=args.emb_sz, n_hid=args.n_hid, n_layers=args.n_layers,
               qrnn=args.qrnn)
    model = get_text_classifier(args.vocab_sz, args.n_class, bptt=args.bptt,
                                max_len=args.max_len, config=cfg) \
        .to(dev, torch.bfloat16).eval()
    ids = torch.randint(9, args.vocab_sz, (args.bs, args.seq_len), device=dev)
    lens = torch.randint(args.seq_len // 4, args.seq_len + 1, (args.bs,),
                         device=dev)
    lens[0] = args.seq_len

    def forward_route():
        with torch.no_grad():
            return torch.sigmoid(model(ids, lens))

    def predict_route():
        return model.predict_proba(ids, lens)[0]

    routes = {"forward": forward_route, "predict_proba": predict_route}
    times = {k: [] for k in routes}
    peak = {}
    out = {}
    for r in range(args.warmup + args.rounds):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            pk = torch.cuda.max_memory_allocated()
            out[name] = res.float()
            del res
            if r >= args.warmup:
                times[name].append(dt)
                peak[name] = {"peak_bytes": pk, "above_baseline_bytes": pk - base}
    res = {"bs": args.bs, "seq_len": args.seq_len, "bptt": args.bptt,
           "max_len": args.max_len,
           "encoder": f"{args.n_layers}x{args.n_hid}/emb{args.emb_sz}"
                      + ("/qrnn" if args.qrnn else ""), "dtype": "bf16",
           "rounds": args.rounds,
           "max_abs_prob_diff": float((out["forward"]
                                       - out["predict_proba"]).abs().max())}
    for name in routes:
        res[name] = {"median_ms": round(statistics.median(times[name]) * 1e3, 2),
                     "min_ms": round(min(times[name]) * 1e3, 2),
                     "max_ms": round(max(times[name]) * 1e3, 2), **peak[name]}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
