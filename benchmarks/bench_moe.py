#!/usr/bin/env python3
"""One MoE feed-forward block: the eager block (MoELayer.forward: torch
routing, a Python loop over the experts with a host read each, hipBLASLt
GEMMs) against the fused one on its two paths: "stream" (moe.hip, the
decode kernels, T * top_k <= 2048) and "tiled" (moe_prefill.hip, the
prefill kernels).

    python benchmarks/bench_moe.py [--tokens 1 8 32 64 128 256 1024 4096]
        [--path stream tiled] [--expert-dtype bf16 fp8] [--rounds 3]
        [--iters 200]

Mixtral 8x7B geometry by default (hidden 4096, inter 14336, E = 8, k = 2).
Per T the contestants alternate for --rounds rounds; a run is --iters calls
between two device events, after a warm-up of all. Every run is listed.
The bytes are those of the gate, up and down weights of the experts the
router actually hit for that input, each counted once; GB/s is those bytes
over the time of one call, next to the 8 TB/s HBM peak of the MI355X. The
FLOPs are those of the routed entries, 6 * T * top_k * hidden * inter;
TFLOP/s next to the 2.5 PFLOP/s dense bf16 MFMA peak. One JSON line per T,
then a summary line.

--expert-dtype fp8 quantises the experts (MoELayer.quantize_experts_: E4M3
bytes and one fp32 scale per weight row); given both, a bf16 and a
quantised copy of the layer alternate in the same rounds and the fp8
contestants carry the suffix _fp8 (their eager block is the dequantising
fallback). A contestant's bytes are the bytes it stores: E4M3 bytes plus
scales for fp8.
"""

import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))

PEAK_GBS = 8000.0
PEAK_TFLOPS = 2500.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tokens", type=int, nargs="+",
                   default=[1, 8, 32, 64, 128, 256, 1024, 4096])
    p.add_argument("--path", nargs="+", choices=["stream", "tiled"],
                   default=["stream", "tiled"],
                   help="the fused paths to run next to the eager block")
    p.add_argument("--no-eager", action="store_true")
    p.add_argument("--expert-dtype", nargs="+", choices=["bf16", "fp8"],
                   default=["bf16"])
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
    # contestant suffix: (layer, stored bytes of one expert)
    layers = {}
    if "bf16" in args.expert_dtype:
        layers[""] = (layer, 3 * args.hidden * args.inter * 2)
    if "fp8" in args.expert_dtype:
        qlayer = copy.deepcopy(layer).quantize_experts_()
        layers["_fp8"] = (qlayer, 3 * args.hidden * args.inter +
                          4 * (2 * args.inter + args.hidden))

    def timed(fn, x):
        beg = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        beg.record()
        for _ in range(args.iters):
            fn(x)
        end.record()
        end.synchronize()
        return beg.elapsed_time(end) / args.iters  # ms per call

    fused_faster = {}
    with torch.no_grad():
        for T in args.tokens:
            x = torch.randn(T, 1, args.hidden, device=dev).to(torch.bfloat16)
            logits = layer.router(x.reshape(T, -1)).float()
            hit = int(K.moe_route(logits, args.top_k)[0].unique().numel())
            fns, nbytes = {}, {}
            for sfx, (lay, eb) in layers.items():
                if not args.no_eager:
                    fns["eager" + sfx] = lay
                for path in args.path:
                    if path == "tiled" or \
                            T * args.top_k <= K.MOE_STREAM_MAX_ENTRIES:
                        fns[path + sfx] = \
                            lambda x, path=path, lay=lay: lay.decode(x, path)
                for n in fns:
                    nbytes.setdefault(n, hit * eb)
            ref = layer(x).float()
            rel = {n: float((fn(x).float() - ref).norm() / ref.norm())
                   for n, fn in fns.items() if n != "eager"}
            for _ in range(3):
                for fn in fns.values():
                    fn(x)
            torch.cuda.synchronize()
            runs = {n: [] for n in fns}
            for _ in range(args.rounds):
                for n, fn in fns.items():
                    runs[n].append(timed(fn, x))
            flops = 6.0 * T * args.top_k * args.hidden * args.inter
            line = {"T": T, "experts_hit": hit,
                    "weight_bytes": nbytes[next(iter(fns))], "flops": flops}
            for n, v in runs.items():
                line[n + "_ms"] = [round(ms, 4) for ms in v]
                line[n + "_weight_bytes"] = nbytes[n]
                line[n + "_GBs"] = [
                    round(nbytes[n] / (ms * 1e-3) / 1e9, 1) for ms in v]
                line[n + "_TFLOPs"] = [round(flops / (ms * 1e-3) / 1e12, 1)
                                       for ms in v]
                if n != "eager":
                    line[n + "_peak_GBs_share"] = round(
                        max(line[n + "_GBs"]) / PEAK_GBS, 3)
                    line[n + "_peak_TFLOPs_share"] = round(
                        max(line[n + "_TFLOPs"]) / PEAK_TFLOPS, 3)
                    line[n + "_vs_eager_rel_l2"] = round(rel[n], 5)
                    if "eager" in runs:
                        faster = max(v) < min(runs["eager"])
                        line["every_%s_run_faster" % n] = faster
                        fused_faster.setdefault(n, []).append((T, faster))
                    if n.endswith("_fp8") and n[:-4] in runs:
                        line["every_%s_run_below_bf16" % n] = \
                            max(v) < min(runs[n[:-4]])
            print(json.dumps(line), flush=True)
    print(json.dumps({
        "metric": "MoE block, fused (stream, tiled) vs eager",
        "every_run_faster_than_every_eager_run_at_T": {
            n: {str(T): f for T, f in v} for n, v in fused_faster.items()},
        "peak_GBs": PEAK_GBS, "peak_TFLOPs": PEAK_TFLOPS,
        "config": {"hidden": args.hidden, "inter": args.inter,
                   "experts": args.experts, "top_k": args.top_k,
                   "rounds": args.rounds, "iters": args.iters},
    }), flush=True)


if __name__ == "__main__":
    main()
