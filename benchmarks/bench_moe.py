#!/usr/bin/env python3
"""One MoE feed-forward block at decode time: the eager block
(MoELayer.forward: torch routing, a Python loop over the experts with a host
read each, hipBLASLt GEMMs) against the fused one (MoELayer.decode: moe.hip).

    python benchmarks/bench_moe.py [--tokens 1 8 32 64] [--rounds 3]
        [--iters 200]

Mixtral 8x7B geometry by default (hidden 4096, inter 14336, E = 8, k = 2).
Per T the two paths alternate for --rounds rounds; a run is --iters calls
between two device events, after a warm-up of both. Every run is listed.
The bytes are those of the gate, up and down weights of the experts the
router actually hit for that input, each counted once; GB/s is those bytes
over the time of one call, next to the 8 TB/s HBM peak of the MI355X. One
JSON line per T, then a summary line.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))

PEAK_GBS = 8000.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tokens", type=int, nargs="+", default=[1, 8, 32, 64])
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--hidden", type=int, default=4096)
    p.add_argument("--inter", type=int, default=14336)
    p.add_argument("--experts", type=int, default=8)
    p.add_argument("--top-k", type=int, default=2)
    args = p.parse_args()

    import torch

    from metaflow_amd.models.mixtral import MixtralConfig, MoELayer
    from metaflow_amd.ops import kernels as K

    assert torch.cuda.is_available(), "bench_moe.py measures on a GPU"
    dev = torch.device("cuda", 0)
    cfg = MixtralConfig(hidden_size=args.hidden,
                        intermediate_size=args.inter,
                        num_experts=args.experts, top_k=args.top_k)
    torch.manual_seed(0)
    with torch.device(dev):
        layer = MoELayer(cfg)
    for prm in layer.parameters():
        torch.nn.init.normal_(prm, std=0.02)
    layer.eval()
    expert_bytes = 3 * args.hidden * args.inter * 2

    def timed(fn, x):
        beg = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        beg.record()
        for _ in range(args.iters):
            fn(x)
        end.record()
        end.synchronize()
        return beg.elapsed_time(end) / args.iters  # ms per call

    all_faster = True
    with torch.no_grad():
        for T in args.tokens:
            x = torch.randn(T, 1, args.hidden, device=dev).to(torch.bfloat16)
            logits = layer.router(x.reshape(T, -1)).float()
            hit = int(K.moe_route(logits, args.top_k)[0].unique().numel())
            ref, out = layer(x).float(), layer.decode(x).float()
            rel = float((out - ref).norm() / ref.norm())
            for _ in range(3):
                layer(x)
                layer.decode(x)
            torch.cuda.synchronize()
            runs = {"eager": [], "fused": []}
            for _ in range(args.rounds):
                runs["eager"].append(timed(layer, x))
                runs["fused"].append(timed(layer.decode, x))
            faster = max(runs["fused"]) < min(runs["eager"])
            all_faster &= faster
            gbs = {n: [hit * expert_bytes / (ms * 1e-3) / 1e9 for ms in v]
                   for n, v in runs.items()}
            print(json.dumps({
                "T": T, "experts_hit": hit,
                "weight_bytes": hit * expert_bytes,
                "eager_ms": [round(v, 4) for v in runs["eager"]],
                "fused_ms": [round(v, 4) for v in runs["fused"]],
                "eager_GBs": [round(v, 1) for v in gbs["eager"]],
                "fused_GBs": [round(v, 1) for v in gbs["fused"]],
                "fused_peak_share": round(max(gbs["fused"]) / PEAK_GBS, 3),
                "every_fused_run_faster": faster,
                "fused_vs_eager_rel_l2": round(rel, 5),
            }), flush=True)
    print(json.dumps({
        "metric": "MoE block, fused vs eager decode",
        "every_fused_run_faster_at_every_T": all_faster,
        "peak_GBs": PEAK_GBS,
        "config": {"hidden": args.hidden, "inter": args.inter,
                   "experts": args.experts, "top_k": args.top_k,
                   "rounds": args.rounds, "iters": args.iters},
    }), flush=True)


if __name__ == "__main__":
    main()
