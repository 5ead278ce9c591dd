"""Fine-tune throughput (examples/s) of the classifier at the reference
notebook's shape: bs=32, deployed 4x2400 encoder (emb 800, vocab 60k), bf16,
at the three unfreezing levels of 06_FineTune.ipynb. Informational; prints
one JSON line.

Usage: python scripts/finetune_bench.py [--seq_len 512 --steps 5 --warmup 2]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from code_intelligence_amd.models.awd_lstm import awd_lstm_lm_config  # noqa: E402
from code_intelligence_amd.models.classifier import get_text_classifier  # noqa: E402
from code_intelligence_amd.train.classifier import ClassifierTrainer  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--bs", type=int, default=32)
    p.add_argument("--seq_len", type=int, default=512)
    p.add_argument("--bptt", type=int, default=70)
    p.add_argument("--max_len", type=int, default=1400)
    p.add_argument("--vocab_sz", type=int, default=60000)
    p.add_argument("--emb_sz", type=int, default=800)
    p.add_argument("--n_hid", type=int, default=2400)
    p.add_argument("--n_layers", type=int, default=4)
    p.add_argument("--n_class", type=int, default=30)
    p.add_argument("--qrnn", action="store_true")
    p.add_argument("--steps", type=int, default=5)
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
        .to(dev, torch.bfloat16)
    tr = ClassifierTrainer(model)
    model.train()
    ids = torch.randint(9, args.vocab_sz, (args.bs, args.seq_len), device=dev)
    lens = torch.randint(args.seq_len // 4, args.seq_len + 1, (args.bs,),
                         device=dev)
    lens[0] = args.seq_len
    y = (torch.rand(args.bs, args.n_class, device=dev) < 0.1).float()
    res = {"bs": args.bs, "seq_len": args.seq_len, "bptt": args.bptt,
           "encoder": f"{args.n_layers}x{args.n_hid}/emb{args.emb_sz}"
                      + ("/qrnn" if args.qrnn else ""), "dtype": "bf16"}
    for name, level in (("frozen", -1), ("freeze_to_-2", -2), ("unfrozen", 0)):
        tr.freeze_to(level)
        lrs = tr.lr_range(slice(1e-4))
        for _ in range(args.warmup):
            loss = tr.train_step(ids, lens, y, lrs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = tr.train_step(ids, lens, y, lrs)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        res[name] = {"ms_per_step": round(dt * 1e3, 2),
                     "examples_per_s": round(args.bs / dt, 2),
                     "loss": round(loss, 4)}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
