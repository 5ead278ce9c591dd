"""Weight-gradient GEMM operand-layout probe (GPU).

Do the K = T*B weight-gradient GEMMs run faster when the small operand is
K-major (contiguous along the reduction), and does the gain survive the
cost of writing that operand? Bench shapes, bf16, device events, 5 warm-up
+ 20 timed calls per variant, three rounds with the variants alternating.

LSTM, per layer shape (In, H), T*B = 262144:
  (a) today's three GEMMs (dgates[0] x h0, dgates[1:] x hs[:-1], dg2 x x)
  (b) one stacked NN GEMM  mm([xT ; hprevT], dg2)  from a pre-built operand
  (c) (b) with dg2 K-major as well: mm(dgT, packed.t())   (information only)
  (d) the pack pass alone (pack_kmajor x3)
  (e) lib.lstm_weight_grads end to end (pack + GEMM + output transposes)
CE, V = 60000, Haug = 816, chunk = 65536:
  (a) mm(dlog.t(), h_aug[s:e])      (b) mm(h_augT[:, s:e], dlog)
  (d) pack of h_aug (N, 816) -> (816, N)

Run: python scripts/dw_layout_probe.py [--out FILE]
"""
import argparse
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
# (a) must run on the kernels the benchmark runs: same tuned-GEMM table
_tun = ROOT / "profiles" / "tunableop_mi355x.csv"
if os.environ.get("PYTORCH_TUNABLEOP_ENABLED") is None:
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = str(_tun)

import torch

from code_intelligence_amd.ops import extension as ext

WARMUP, ITERS, ROUNDS = 5, 20, 3


def time_ms(fn):
    for _ in range(WARMUP):
        fn()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / ITERS


def run_rounds(variants):
    """variants: {name: fn}. Returns {name: [ms per round]}, alternating."""
    res = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            res[k].append(time_ms(fn))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--B", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f"{__file__} is a GPU probe - run it on an MI355X")
    lib = ext.require()
    dev, dt = "cuda:0", torch.bfloat16
    torch.manual_seed(0)
    T, B = args.T, args.B
    K = T * B
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# dw_layout_probe T={T} B={B} K={K} bf16, ms = mean of "
         f"{ITERS} calls, {ROUNDS} alternating rounds")
    emit("| case | variant | ms (rounds) | median ms | TF/s or GB/s |")
    emit("|---|---|---|---|---|")
    for In, H in ((800, 2400), (2400, 2400), (2400, 800)):
        G = 4 * H
        dgates = torch.randn(T, B, G, device=dev, dtype=dt)
        x = torch.randn(T, B, In, device=dev, dtype=dt)
        hs = torch.randn(T, B, H, device=dev, dtype=dt)
        h0 = torch.randn(B, H, device=dev, dtype=dt)
        dg2 = dgates.view(K, G)
        packed = torch.empty(In + H, K, device=dev, dtype=dt)
        dgT = dg2.t().contiguous()

        def pack():
            lib.pack_kmajor(x.view(K, In), packed, 0, 0)
            lib.pack_kmajor(h0, packed, In, 0)
            lib.pack_kmajor(hs[:-1].view((T - 1) * B, H), packed, In, B)

        def three():
            dw_hh = torch.mm(dgates[0].t(), h0)
            dw_hh += torch.mm(dgates[1:].reshape((T - 1) * B, G).t(),
                              hs[:-1].reshape((T - 1) * B, H))
            return dw_hh, torch.mm(dg2.t(), x.view(K, In))

        pack()
        # same values both ways before anything is timed
        ref_hh, ref_ih = three()
        got_ih, got_hh = lib.lstm_weight_grads(dgates, x, hs, h0)
        for name, r, g in (("ih", ref_ih, got_ih), ("hh", ref_hh, got_hh)):
            rel = ((r.float() - g.float()).abs().max()
                   / r.float().abs().max()).item()
            emit(f"<!-- ({In},{H}) dw_{name} max|diff|/max|ref| = {rel:.2e} -->")
        del ref_hh, ref_ih, got_ih, got_hh
        res = run_rounds({
            "a: three Ailk_Bjlk GEMMs": three,
            "b: mm(packed, dg2)": lambda: torch.mm(packed, dg2),
            "c: mm(dgT, packed.t())": lambda: torch.mm(dgT, packed.t()),
            "d: pack x3": pack,
            "e: lstm_weight_grads": lambda: lib.lstm_weight_grads(
                dgates, x, hs, h0),
        })
        flop = 2.0 * K * G * (In + H)
        byts = 2.0 * K * (In + H) * 2  # read + write floor of the pack
        for k, v in res.items():
            med = sorted(v)[len(v) // 2]
            rate = (f"{byts / med / 1e6:.0f} GB/s" if k.startswith("d")
                    else f"{flop / med / 1e9:.0f} TF/s")
            emit(f"| LSTM In={In} H={H} | {k} | "
                 f"{', '.join(f'{t:.2f}' for t in v)} | {med:.2f} | {rate} |")
        del dgates, x, hs, h0, dg2, packed, dgT
        torch.cuda.empty_cache()

    # ---- CE dW -----------------------------------------------------------
    V, Haug, C, N = 60000, 816, 65536, K
    dlog = torch.randn(C, V, device=dev, dtype=dt)
    h_aug = torch.randn(N, Haug, device=dev, dtype=dt)
    h_augT = torch.empty(Haug, N, device=dev, dtype=dt)
    lib.pack_kmajor(h_aug, h_augT, 0, 0)
    s, e = C, 2 * C
    res = run_rounds({
        "a: mm(dlog.t(), h_aug[s:e])": lambda: torch.mm(dlog.t(), h_aug[s:e]),
        "b: mm(h_augT[:, s:e], dlog)": lambda: torch.mm(h_augT[:, s:e], dlog),
        "d: pack h_aug (N,816)": lambda: lib.pack_kmajor(h_aug, h_augT, 0, 0),
    })
    flop = 2.0 * C * V * Haug
    byts = 2.0 * N * Haug * 2
    for k, v in res.items():
        med = sorted(v)[len(v) // 2]
        rate = (f"{byts / med / 1e6:.0f} GB/s" if k.startswith("d")
                else f"{flop / med / 1e9:.0f} TF/s")
        emit(f"| CE chunk={C} | {k} | {', '.join(f'{t:.2f}' for t in v)} "
             f"| {med:.2f} | {rate} |")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
