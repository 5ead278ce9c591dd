"""Beam-search benchmark: ms per word at the deployed shape.

Compares, in one process and alternating between the two,
  k11   : AWDLSTM.beam_search (topk_logprobs + beam_select, token / parent /
          score buffers on the device, one host copy at the end)
  eager : fastai's loop on this project's encoder, i.e. F.linear +
          log_softmax + topk + argsort + torch.cat of the node prefixes +
          select_hidden per word
at top_k = 10 and beam_sz in {10, 100, 1000}, and reports the median over
repeats, the spread of each, and the share of a word taken by the two K11
launches (timed alone with device events at the steady-state row count).

--sweep also times the two logits paths of beam_search against each other,
ops.decode_logits and one library GEMM, at 1..128 rows: the crossover constant
models.awd_lstm.BEAM_GEMM_CROSSOVER is the largest row count at which the GEMM
does not yet win by more than the spread.

    python scripts/beam_bench.py [--repeats 5] [--words 32] [--prompt 32] [--sweep]

Prints one JSON line. Needs a GPU: there is no CPU fallback for a timing.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def eager_beam_search(model, prompt, n_words, top_k, beam_sz, unk):
    xb = prompt
    nodes = prompt.clone()
    scores = prompt.new_zeros(1).float()
    lin = model.decoder.decoder
    with torch.no_grad():
        model.reset(1)
        for _ in range(n_words):
            h = model.encoder(xb)[1][-1][:, -1]
            out = F.log_softmax(F.linear(h, lin.weight, lin.bias).float(),
                                dim=-1)
            out[:, unk] = -float("inf")
            values, indices = out.topk(top_k, dim=-1)
            scores = (-values + scores[:, None]).view(-1)
            n = nodes.size(0)
            indices_idx = torch.arange(0, n, device=prompt.device)[:, None] \
                .expand(n, top_k).contiguous().view(-1)
            sort_idx = scores.argsort()[:beam_sz]
            scores = scores[sort_idx]
            nodes = torch.cat(
                [nodes[:, None].expand(n, top_k, nodes.size(1)),
                 indices[:, :, None].expand(n, top_k, 1)], dim=2)
            nodes = nodes.view(-1, nodes.size(2))[sort_idx]
            model.encoder.select_hidden(indices_idx[sort_idx])
            xb = nodes[:, -1][:, None]
    node_idx = torch.multinomial(torch.exp(-(scores - scores.min())), 1).item()
    return nodes[node_idx][prompt.size(1):].tolist()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def stats(xs):
    return {"median": round(statistics.median(xs), 4),
            "min_max": [round(min(xs), 4), round(max(xs), 4)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--words", type=int, default=32)
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--vocab", type=int, default=60000)
    ap.add_argument("--top_k", type=int, default=10)
    ap.add_argument("--beams", type=int, nargs="*", default=[10, 100, 1000])
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_bench needs a GPU")
    from code_intelligence_amd.models import awd_lstm
    from code_intelligence_amd.ops import (beam_select, decode_logits,
                                           topk_logprobs)
    dev = "cuda:0"
    torch.manual_seed(0)
    model = awd_lstm.AWDLSTM(vocab_sz=args.vocab, emb_sz=800, n_hid=2400,
                             n_layers=4) \
        .to(device=dev, dtype=torch.bfloat16).eval()
    lin = model.decoder.decoder
    result = {"shape": f"V{args.vocab} emb800 4x2400 bf16",
              "prompt": args.prompt, "words": args.words, "top_k": args.top_k,
              "crossover": awd_lstm.BEAM_GEMM_CROSSOVER, "beams": {}}
    prompt = torch.randint(10, args.vocab, (1, args.prompt), device=dev)
    for beam_sz in args.beams:
        k11 = lambda: model.beam_search(prompt, args.words, top_k=args.top_k,
                                        beam_sz=beam_sz, seed=1)
        eager = lambda: eager_beam_search(model, prompt, args.words,
                                          args.top_k, beam_sz, 0)
        for _ in range(2):                  # warm every shape of both loops
            k11()
            eager()
        tk, te = [], []
        for _ in range(args.repeats):       # alternate the two
            tk.append(timed(k11) / args.words)
            te.append(timed(eager) / args.words)
        # the two K11 launches alone, at the steady-state row count
        B = beam_sz
        h = torch.randn(B, 800, device=dev).to(torch.bfloat16)
        if B <= awd_lstm.BEAM_GEMM_CROSSOVER:
            logits, _ = decode_logits(h, lin.weight, lin.bias)
        else:
            logits = F.linear(h, lin.weight, lin.bias)
        scores = torch.rand(B, device=dev)
        n_out = min(beam_sz, B * args.top_k)
        vi = (torch.empty(B, args.top_k, device=dev),
              torch.empty(B, args.top_k, dtype=torch.int64, device=dev))
        out = (torch.empty(n_out, device=dev),
               torch.empty(n_out, dtype=torch.int64, device=dev),
               torch.empty(n_out, dtype=torch.int64, device=dev))

        def launches():
            topk_logprobs(logits, args.top_k, 0, out=vi)
            beam_select(scores, vi[0], vi[1], beam_sz, out=out)
        event_ms(launches, 10)
        both = event_ms(launches, 100)
        topk_only = event_ms(
            lambda: topk_logprobs(logits, args.top_k, 0, out=vi), 100)
        mk = statistics.median(tk)
        result["beams"][str(beam_sz)] = {
            "k11_ms_per_word": stats(tk), "eager_ms_per_word": stats(te),
            "k11_launches_ms_per_word": round(both, 4),
            "topk_logprobs_ms": round(topk_only, 4),
            "k11_launch_share_of_word": round(both / mk, 3),
        }
    if args.sweep:
        result["logits_sweep"] = {}
        for B in (1, 2, 4, 8, 16, 32, 64, 128):
            h = torch.randn(B, 800, device=dev).to(torch.bfloat16)
            scratch = decode_logits(h, lin.weight, lin.bias)
            gemv = lambda: decode_logits(h, lin.weight, lin.bias, out=scratch)
            gemm = lambda: F.linear(h, lin.weight, lin.bias)
            event_ms(gemv, 10)
            event_ms(gemm, 10)
            tv, tg = [], []
            for _ in range(args.repeats):   # alternate the two
                tv.append(event_ms(gemv, 50))
                tg.append(event_ms(gemm, 50))
            result["logits_sweep"][str(B)] = {
                "decode_logits_ms": stats(tv), "gemm_ms": stats(tg)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
