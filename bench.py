#!/usr/bin/env python3
"""Flagship benchmark: AWD-LSTM LM pretraining step on MI355X.

Measures the BASELINE.json headline metric — LM tokens/sec (whole node) —
on the reference's deployed model config (AWD-LSTM n_layers=4, n_hid=2400,
emb_sz=800, vocab 60k — BASELINE.md 'Deployed LM architecture') with
synthetic issue-text tokens and random-init weights, bf16 compute,
per-GPU batch 512 x seq 512 (BASELINE.json configs 2-3: global bs 4096 at
DP=8, weak scaling).

Single GPU:      python bench.py --gpus 1 --steps 20 --warmup 5
                 (plain run: set up, warm up, time the steps, print the line)
Everything else: add --full (quick serve sub-benchmark in the same line)
Outputs:         add --dump-outputs DIR (last timed step, as DIR/<name>.npy)
Multi GPU (DP):  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
                     --master-addr 127.0.0.1 bench.py --gpus N ...
"""
from __future__ import annotations

import argparse
import json
import os
import time
from pathlib import Path

# Ship-time hipBLASLt solution selection: load the pre-tuned TunableOp
# results for MI355X if present (tuned once offline; +2% step time, no
# runtime tuning). Must be set before torch initializes.
_tun = Path(__file__).resolve().parent / "profiles" / "tunableop_mi355x.csv"
if _tun.with_name("tunableop_mi355x0.csv").exists()         and os.environ.get("PYTORCH_TUNABLEOP_ENABLED") is None:
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = str(_tun)

import torch

from code_intelligence_amd.data.synthetic import synthetic_issue_tokens
from code_intelligence_amd.models.awd_lstm import AWDLSTM
from code_intelligence_amd.parallel.ddp import init_distributed
from code_intelligence_amd.train.trainer import LMTrainer, TrainConfig


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--bs", type=int, default=512)        # per-GPU
    p.add_argument("--seq", type=int, default=512)
    p.add_argument("--vocab", type=int, default=60000)
    p.add_argument("--emb", type=int, default=800)
    p.add_argument("--hid", type=int, default=2400)
    p.add_argument("--layers", type=int, default=4)
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--qrnn", type=lambda v: v.lower() == "true", default=False,
                   help="bench the QRNN encoder variant (not the headline config)")
    p.add_argument("--lstm_mode", type=str, default=None,
                   help="override CI_LSTM_MODE (fused|lib)")
    p.add_argument("--serve", action="store_true",
                   help="serve-only mode: print the issue-embeddings/sec "
                        "JSON line instead of the LM training line")
    p.add_argument("--no-serve", action="store_true",
                   help="skip the serve sub-benchmark in the LM line")
    p.add_argument("--full", action="store_true",
                   help="also run everything beyond the headline figure "
                        "(the quick serve sub-benchmark carried in the LM "
                        "line); off by default so a plain run stays lean")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps write what the last timed "
                        "step computed (loss, hidden state, updated "
                        "parameters) as DIR/<name>.npy")
    return p.parse_args()


def serve_bench(args, quick: bool = True) -> dict:
    """Driver-timed serve metric (BASELINE.json 'issue-embeddings/sec
    served', config 4): bulk batched path + single-request latency on the
    deployed shape, synthetic issues, random-init weights."""
    import numpy as np
    from code_intelligence_amd.data.synthetic import synthetic_issue_texts
    from code_intelligence_amd.engine.inference import InferenceWrapper
    from code_intelligence_amd.text.tokenizer import Vocab, defaults_specials

    torch.manual_seed(0)
    on_gpu = torch.cuda.is_available()
    emb, hid, layers, vocab = (args.emb, args.hid, args.layers, args.vocab) \
        if on_gpu else (400, 400, 3, 30000)
    words = [f"w{i}" for i in range(vocab - len(defaults_specials))]
    v = Vocab(defaults_specials + words)
    from code_intelligence_amd.models.awd_lstm import AWDLSTM
    model = AWDLSTM(vocab_sz=len(v), emb_sz=emb, n_hid=hid, n_layers=layers,
                    qrnn=args.qrnn)
    w = InferenceWrapper(encoder=model.encoder, vocab=v,
                         use_graphs=os.environ.get("CI_SERVE_GRAPHS",
                                                   "0") == "1")
    n_bulk, n_single = (1500, 30) if quick else (2000, 100)
    if not on_gpu:
        n_bulk, n_single = 40, 5
    issues = synthetic_issue_texts(n_bulk, seed=3)
    texts = [w.process_dict(d)["text"] for d in issues]
    # warm up with the SAME batch size as the timed run so first-use
    # bucket shapes (hipBLASLt solution selection) stay out of the timing
    w.texts_to_embedding(texts[:min(256, n_bulk)], bs=200)
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = w.texts_to_embedding(texts, bs=200)
    if on_gpu:
        torch.cuda.synchronize()
    bulk_dt = time.perf_counter() - t0
    lat = []
    for d in issues[:n_single]:
        t0 = time.perf_counter()
        w.get_pooled_features(w.process_dict(d)["text"])
        if on_gpu:
            torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
    lat.sort()
    return {
        "embeddings_per_sec_bulk": round(n_bulk / bulk_dt, 1),
        "model": f"AWD-{'QRNN' if args.qrnn else 'LSTM'} {layers}x{hid} "
                 f"emb{emb} vocab{vocab}",
        "bulk_n": n_bulk, "bulk_bs": 200, "dim": int(out.shape[1]),
        "single_p50_ms": round(lat[len(lat) // 2] * 1e3, 2),
        "single_p95_ms": round(lat[min(len(lat) - 1,
                                       int(len(lat) * 0.95))] * 1e3, 2),
    }


# per-tensor element cap of --dump-outputs: ~30 tensors x 256k x 4 B stays
# far below 64 MB for any model size
_DUMP_MAX_ELEMS = 1 << 18


def dump_outputs(out_dir: str, loss: float, model) -> None:
    """Write what a caller of the timed path holds after its last step: the
    step's loss, the carried hidden state and the updated parameters.
    float32 .npy (loss float64); tensors above _DUMP_MAX_ELEMS elements are
    reduced to a fixed seeded sample of their flattened elements, the same
    indices on every run."""
    import numpy as np
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    np.save(d / "loss.npy", np.asarray([loss], dtype=np.float64))
    named = [(f"param.{n}", p) for n, p in model.named_parameters()]
    for l, (h, c) in enumerate(model.encoder.hidden):
        named += [(f"hidden.{l}.h", h), (f"hidden.{l}.c", c)]
    g = torch.Generator().manual_seed(4321)
    for name, t in named:
        flat = t.detach().reshape(-1)
        if flat.numel() > _DUMP_MAX_ELEMS:
            idx = torch.randint(0, flat.numel(), (_DUMP_MAX_ELEMS,),
                                generator=g).sort().values
            flat = flat[idx.to(flat.device)]
        np.save(d / f"{name}.npy", flat.float().cpu().numpy())


def main():
    args = parse_args()
    if args.lstm_mode:
        os.environ["CI_LSTM_MODE"] = args.lstm_mode
    if args.serve:
        s = serve_bench(args, quick=False)
        print(json.dumps({
            "metric": "issue-embeddings/sec served",
            "value": s["embeddings_per_sec_bulk"],
            "unit": "embeddings/s", "n_gpus": 1,
            "steps": s["bulk_n"], "warmup": 128,
            "ms_per_step": round(1000.0 / max(s["embeddings_per_sec_bulk"],
                                              1e-9), 3),
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {
                "model": s["model"],
                "global_batch": s["bulk_bs"], "seq_len": "variable",
                "parallelism": "serve-1gpu",
                "single_p50_ms": s["single_p50_ms"],
                "single_p95_ms": s["single_p95_ms"],
            }}))
        return
    rank, world = init_distributed()
    on_gpu = torch.cuda.is_available()
    serve = None
    if args.full and rank == 0 and world == 1 and not args.no_serve:
        # BASELINE.json's metric names BOTH halves ("LM tokens/sec ... and
        # issue-embeddings/sec served"): measure serving FIRST, before the
        # sustained training burst drags clocks down.
        serve = serve_bench(args, quick=True)
        if on_gpu:
            torch.cuda.empty_cache()
    if not on_gpu:
        # CPU fallback: plumbing config (BASELINE.json config 1) so the
        # script stays runnable off-GPU; the official metric is GPU-only.
        args.bs, args.seq, args.vocab = 2, 64, 30000
        args.emb, args.hid, args.layers = 400, 400, 3
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0))) \
        if on_gpu else torch.device("cpu")
    dtype = torch.bfloat16 if (args.dtype == "bf16" and on_gpu) else torch.float32

    torch.manual_seed(1234 + rank)
    model = AWDLSTM(vocab_sz=args.vocab, emb_sz=args.emb, n_hid=args.hid,
                    n_layers=args.layers, qrnn=args.qrnn
                    ).to(device=device, dtype=dtype)
    trainer = LMTrainer(model, TrainConfig(), distributed=(world > 1))
    model.train()
    model.reset(args.bs)

    # synthetic issue-shaped stream, pre-batched on device
    docs = synthetic_issue_tokens(64, args.vocab, seed=7 + rank, mean_len=300)
    stream = torch.tensor([t for d in docs for t in d], dtype=torch.int64)
    need = args.bs * (args.seq + 1) * (args.steps + args.warmup)
    reps = need // stream.numel() + 1
    stream = stream.repeat(reps)[:need].view(-1, args.seq + 1).to(device)

    def batch(i):
        s = (i * args.bs) % (stream.shape[0] - args.bs + 1)
        win = stream[s: s + args.bs]
        return win[:, :-1], win[:, 1:]

    lr = trainer.cfg.lr
    for i in range(args.warmup):
        x, y = batch(i)
        trainer.train_step(x, y, lr)

    def barrier_sync():
        if world > 1:
            torch.distributed.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    barrier_sync()
    last_loss = float("nan")
    t0 = time.perf_counter()
    for i in range(args.steps):
        x, y = batch(args.warmup + i)
        last_loss = trainer.train_step(x, y, lr)
    barrier_sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=device if on_gpu else None)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t)

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_loss, model)

    n_gpus = world if on_gpu else args.gpus
    tokens = args.bs * args.seq * args.steps * world
    value = tokens / elapsed

    if rank == 0:
        print(json.dumps({
            "metric": "LM tokens/sec (whole node)",
            "value": round(value, 1),
            "unit": "tokens/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if dtype == torch.bfloat16 else "fp32",
            "data": "synthetic",
            "config": {
                "model": f"AWD-{'QRNN' if args.qrnn else 'LSTM'} {args.layers}x{args.hid} emb{args.emb} vocab{args.vocab}",
                "global_batch": args.bs * world,
                "seq_len": args.seq,
                "parallelism": f"dp{world}",
                "device": "MI355X" if on_gpu else "cpu-fallback",
            },
            **({"serve": serve} if serve is not None else {}),
        }))
    if world > 1 and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
