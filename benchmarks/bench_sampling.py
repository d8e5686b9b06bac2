#!/usr/bin/env python3
"""Token selection at Llama-3 vocabulary: the fused sampler
(ops/csrc/sampling.hip) against what it replaces.

    python benchmarks/bench_sampling.py [--iters 50] [--rounds 3]

V = 128 256, bf16 logits [B, 1, V] as a decode step returns them,
B in {1, 8, 32}. Every figure is WALL time per selection including the
host read that delivers the ids. Per (B, configuration) the kernel and its
baseline run in alternating rounds and every run is listed:

  greedy       K.sample_tokens(temperature 0) + one .tolist()
               vs the per-slot `int(logits[i, -1].float().argmax())` loop
  top-k 50, top-p 0.9, both
               K.sample_tokens + one .tolist()
               vs a sampler composed of torch ops on the device (softmax,
               sort, cumsum, mask, inverse CDF) + one .tolist()

One JSON line per (B, configuration); "kernel_below_baseline" says
whether every kernel run was below every baseline run.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))

V = 128256
# (name, temperature, top_k, top_p)
CONFIGS = [("greedy", 0.0, 0, 1.0), ("top_k_50", 1.0, 50, 1.0),
           ("top_p_0.9", 1.0, 0, 0.9), ("top_k_50_top_p_0.9", 1.0, 50, 0.9)]


def per_slot_argmax(logits):
    """The engine's selection before the fused sampler, verbatim."""
    out = []
    for i in range(logits.size(0)):
        nxt = int(logits[i, -1].float().argmax())
        out.append(nxt)
    return out


def torch_sampler(logits, temperature, top_k, top_p, u):
    import torch

    x = logits[:, -1].float() / temperature
    vals, idx = x.sort(dim=-1, descending=True)
    if top_k:
        vals[:, top_k:] = float("-inf")
    probs = torch.softmax(vals, dim=-1)
    if top_p < 1:
        cum = probs.cumsum(dim=-1)
        probs = probs.masked_fill(cum - probs >= top_p, 0.0)
        probs = probs / probs.sum(dim=-1, keepdim=True)
    cdf = probs.cumsum(dim=-1)
    pos = (cdf <= u[:, None]).sum(dim=-1).clamp(max=x.size(1) - 1)
    return idx.gather(1, pos[:, None])[:, 0].tolist()


def timed(fn, iters):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    args = p.parse_args()

    import torch

    from metaflow_amd.ops import kernels as K

    dev = "cuda"
    torch.manual_seed(0)
    for B in args.batches:
        logits = (torch.randn(B, 1, V, device=dev) * 3).to(torch.bfloat16)
        u = torch.rand(B, device=dev)
        for name, T, k, tp in CONFIGS:
            temp_t = torch.full((B,), T, device=dev)
            k_t = torch.full((B,), k, dtype=torch.int32, device=dev)
            p_t = torch.full((B,), tp, device=dev)

            def kernel():
                return K.sample_tokens(logits[:, -1], temp_t, k_t, p_t,
                                       u).tolist()

            if T <= 0:
                def baseline():
                    return per_slot_argmax(logits)
                assert kernel() == baseline()
            else:
                def baseline():
                    return torch_sampler(logits, T, k, tp, u)
            runs_k, runs_b = [], []
            for _ in range(args.rounds):
                runs_k.append(round(timed(kernel, args.iters), 1))
                runs_b.append(round(timed(baseline, args.iters), 1))
            print(json.dumps({
                "metric": "token selection wall time", "unit": "us",
                "B": B, "V": V, "config": name,
                "kernel_us": runs_k, "baseline_us": runs_b,
                "baseline": ("per-slot argmax loop" if T <= 0
                             else "torch-composed sampler"),
                "kernel_below_baseline": max(runs_k) < min(runs_b),
            }), flush=True)


if __name__ == "__main__":
    main()
