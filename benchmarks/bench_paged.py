#!/usr/bin/env python3
"""Paged decode: K.attn_decode_paged against K.attn_decode_varlen (the
paged and the dense instantiation of ops/csrc/decode.hip) on identical
cache contents, same device. The two kernels are one body; the comparison
isolates the block-table indirection and the page-aligned split.

    python benchmarks/bench_paged.py [--iters 50] [--warmup 5]

Fixed shapes, H=32, Hkv=8 (Llama-8B attention), every sequence full:
    batch   B=8  L=4096
    long    B=1  L=16384
Each shape runs with pages handed out in order (the pool is then the
contiguous cache, re-tiled) and randomly permuted, plus one diagnostic
order: runs of 16 pages (2 MiB per pool tensor) shuffled, in order within
a run, which separates the cost of scattered memory from the cost of the
table lookup. One JSON line per run:
device-event time per call of both kernels (best of 3 alternating runs of
`iters` calls, with the three runs listed), paged/contiguous, GB/s over
the cache stream (K and V rows of the Hkv heads, once) and the worst
per-row relative difference between the two outputs. Needs a GPU: a CPU
timing says nothing about the kernel.
"""

import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))

H, HKV, D, PAGE = 32, 8, 128, 64
SHAPES = [("batch", 8, 4096), ("long", 1, 16384)]
# pages per 2 MiB of one pool tensor (a page is Hkv * 64 * 128 bf16)
GROUP = (2 << 20) // (HKV * PAGE * D * 2)


def _time_ms(fn, warmup, iters):
    """Mean device time per call: events around `iters` back-to-back
    calls, after `warmup` calls of the same shape."""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    args = p.parse_args()

    import torch

    from metaflow_amd.ops import kernels as K

    if not torch.cuda.is_available():
        sys.exit("bench_paged.py measures the GPU kernel: no GPU found")
    dev = torch.device("cuda", 0)
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(0)

    for name, B, L in SHAPES:
        pps = L // PAGE
        q = torch.randn(B, H, 1, D, device=dev, dtype=torch.bfloat16)
        kc = torch.randn(B, HKV, L, D, device=dev, dtype=torch.bfloat16)
        vc = torch.randn(B, HKV, L, D, device=dev, dtype=torch.bfloat16)
        lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
        stream_bytes = 2 * B * HKV * L * D * 2

        def contiguous():
            return K.attn_decode_varlen(q, kc, vc, lengths, scale,
                                        max_len=L)

        for order in ("in order", "permuted", "permuted 2 MiB groups"):
            n = B * pps
            if order == "in order":
                perm = torch.arange(n)
            elif order == "permuted":
                perm = torch.randperm(n)
            else:
                # diagnostic: shuffle runs of GROUP pages (2 MiB of K),
                # pages in order within a run — the same table lookups,
                # coarser physical scatter
                perm = (torch.randperm(n // GROUP)[:, None] * GROUP
                        + torch.arange(GROUP)[None, :]).reshape(-1)
            table = perm.view(B, pps).to(device=dev, dtype=torch.int32)
            # page table[b, j] <- rows 64j..64j+63 of sequence b
            src_k = kc.view(B, HKV, pps, PAGE, D).permute(0, 2, 1, 3, 4)
            src_v = vc.view(B, HKV, pps, PAGE, D).permute(0, 2, 1, 3, 4)
            kp = torch.empty(n, HKV, PAGE, D, device=dev,
                             dtype=torch.bfloat16)
            vp = torch.empty_like(kp)
            idx = table.view(-1).long()
            kp[idx] = src_k.reshape(n, HKV, PAGE, D)
            vp[idx] = src_v.reshape(n, HKV, PAGE, D)

            def paged():
                return K.attn_decode_paged(q, kp, vp, table, lengths,
                                           scale, L)

            o, ref = paged().float(), contiguous().float()
            row_err = ((o - ref).norm(dim=-1)
                       / ref.norm(dim=-1)).max().item()
            # alternate the two kernels so drift hits both alike
            t_p, t_c = [], []
            for _ in range(3):
                t_p.append(_time_ms(paged, args.warmup, args.iters))
                t_c.append(_time_ms(contiguous, args.warmup, args.iters))
            p_ms, c_ms = min(t_p), min(t_c)
            print(json.dumps({
                "metric": "attn_decode_paged ms/call", "shape": name,
                "pages": order, "value": round(p_ms, 4), "unit": "ms",
                "higher_is_better": False,
                "contiguous_ms": round(c_ms, 4),
                "paged_over_contiguous": round(p_ms / c_ms, 3),
                "paged_ms_runs": [round(t, 4) for t in t_p],
                "contiguous_ms_runs": [round(t, 4) for t in t_c],
                "paged_GBps": round(stream_bytes / p_ms / 1e6, 1),
                "contiguous_GBps": round(stream_bytes / c_ms / 1e6, 1),
                "worst_row_rel_diff": float("%.3e" % row_err),
                "config": {"B": B, "H": H, "Hkv": HKV, "L": L},
            }), flush=True)
            del kp, vp
        del q, kc, vc


if __name__ == "__main__":
    main()
