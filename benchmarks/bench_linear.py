#!/usr/bin/env python3
"""The dense projections of a Llama-3-8B decode step, one at a time: the
bf16 GEMM the model runs today against the weight stream of linear_fp8.hip.

    python benchmarks/bench_linear.py [--rows 1 8 32 64 128 256]
        [--shapes qkv o gate_up down lm_head] [--rounds 3] [--window-ms 250]
        [--splits N]

Contestants per (shape, M):
  tuned_bf16   ops.gemm.tuned_linear on bf16 weights (+ K.swiglu_fused for
               gate|up): what LlamaForCausalLM runs unquantised
  stream_bf16  K.linear_w8 on the same bf16 weights: what the kernel buys
  stream_fp8   K.linear_w8 on E4M3 bytes and row scales: what the bytes buy
  dequant_fp8  K.linear_dequant + tuned_linear (+ swiglu_fused): the
               fallback of Fp8WeightLinear above STREAM_MAX_ROWS

They alternate for --rounds rounds after a warm-up of all; a run is a window
of about --window-ms between two device events, and every run is listed. One
weight fits the 256 MB last-level cache, so every contestant cycles through
enough distinct copies of its weight that a pass over them reads more than
--cycle-gb (1.5) GB before one repeats: the GB/s are HBM figures. Bytes are
the stored weight bytes plus scales of one call. One JSON line per (shape,
M), then a summary line."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))

PEAK_GBS = 8000.0
# name: (out rows, in, swiglu) at Llama-3-8B geometry
SHAPES = {"qkv": (6144, 4096, False), "o": (4096, 4096, False),
          "gate_up": (28672, 4096, True), "down": (4096, 14336, False),
          "lm_head": (128256, 4096, False)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, nargs="+",
                   default=[1, 8, 32, 64, 128, 256])
    p.add_argument("--shapes", nargs="+", choices=sorted(SHAPES),
                   default=["qkv", "o", "gate_up", "down", "lm_head"])
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--window-ms", type=float, default=250.0)
    p.add_argument("--cycle-gb", type=float, default=1.5)
    p.add_argument("--splits", type=int, default=None,
                   help="split of K for the stream kernels (default: the "
                        "shape rule)")
    args = p.parse_args()

    import torch

    from metaflow_amd.ops import kernels as K
    from metaflow_amd.ops.gemm import tuned_linear

    assert torch.cuda.is_available(), "bench_linear.py measures on a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)

    def window(fn, copies, x, iters):
        beg = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        beg.record()
        for i in range(iters):
            fn(x, *copies[i % len(copies)])
        end.record()
        end.synchronize()
        return beg.elapsed_time(end) / iters  # ms per call

    summary = {}
    with torch.no_grad():
        for name in args.shapes:
            rows, kdim, swiglu = SHAPES[name]
            b16, b8 = rows * kdim * 2, rows * kdim + rows * 4
            n16 = max(2, int(args.cycle_gb * 1e9 / b16) + 1)
            n8 = max(2, int(args.cycle_gb * 1e9 / b8) + 1)
            base = torch.randn(rows, kdim, device=dev) * 0.02
            w16 = [(base * (1 + 0.01 * i)).to(torch.bfloat16)
                   for i in range(n16)]
            w8 = [K.moe_quant_weight(base * (1 + 0.01 * i))
                  for i in range(n8)]
            del base

            def tuned(x, w):
                y = tuned_linear(x, w)
                return K.swiglu_fused(y) if swiglu else y

            def stream(x, w, s=None):
                return K.linear_w8(x, w, s, swiglu=swiglu,
                                   splits=args.splits)

            def dequant(x, w, s):
                return tuned(x, K.linear_dequant(w, s))

            # contestant: (fn, weight copies, stored bytes of one call)
            fns = {"tuned_bf16": (tuned, [(w,) for w in w16], b16),
                   "stream_bf16": (stream, [(w,) for w in w16], b16),
                   "stream_fp8": (stream, w8, b8),
                   "dequant_fp8": (dequant, w8, b8)}
            for M in args.rows:
                x = torch.randn(M, kdim, device=dev).to(torch.bfloat16)
                ref = tuned(x, w16[0]).float()
                rel = float((stream(x, *w8[0]).float() - ref).norm()
                            / ref.norm())
                iters = {}
                for n, (fn, copies, _) in fns.items():
                    window(fn, copies, x, len(copies))       # warm-up
                    ms = window(fn, copies, x, len(copies))
                    iters[n] = max(len(copies),
                                   int(args.window_ms / max(ms, 1e-3)))
                runs = {n: [] for n in fns}
                for _ in range(args.rounds):
                    for n, (fn, copies, _) in fns.items():
                        runs[n].append(window(fn, copies, x, iters[n]))
                line = {"shape": name, "out": rows, "in": kdim,
                        "swiglu": swiglu, "M": M,
                        "stream_fp8_vs_bf16_rel_l2": round(rel, 5)}
                for n, v in runs.items():
                    nb = fns[n][2]
                    line[n + "_ms"] = [round(ms, 4) for ms in v]
                    line[n + "_iters"] = iters[n]
                    line[n + "_copies"] = len(fns[n][1])
                    line[n + "_GBs"] = [
                        round(nb / (ms * 1e-3) / 1e9, 1) for ms in v]
                    line[n + "_peak_share"] = round(
                        max(line[n + "_GBs"]) / PEAK_GBS, 3)
                for n in ("stream_bf16", "stream_fp8"):
                    line["every_%s_run_below_tuned" % n] = \
                        max(runs[n]) < min(runs["tuned_bf16"])
                line["every_stream_fp8_run_below_dequant"] = \
                    max(runs["stream_fp8"]) < min(runs["dequant_fp8"])
                summary.setdefault(name, {})[str(M)] = \
                    line["every_stream_fp8_run_below_tuned"]
                print(json.dumps(line), flush=True)
            del w16, w8, fns
            torch.cuda.empty_cache()
    print(json.dumps({
        "metric": "dense projections, stream (bf16, fp8) vs tuned bf16 GEMM",
        "every_stream_fp8_run_below_every_tuned_run": summary,
        "peak_GBs": PEAK_GBS,
        "config": {"rounds": args.rounds, "window_ms": args.window_ms,
                   "cycle_gb": args.cycle_gb, "splits": args.splits},
    }), flush=True)


if __name__ == "__main__":
    main()
