#!/usr/bin/env python3
"""Append attention: K.attn_append (ops/csrc/append.hip) against the eager
fp32 path it replaces (K.attn_append_ref), same device, same inputs.

    python benchmarks/bench_append.py [--iters 50] [--warmup 5]

Fixed shapes, all H=32, Hkv=8, B=1 (Llama-8B attention):
    verify      Sq=5    pos=4096    speculative verification block
    chunk       Sq=512  pos=3584    chunked prefill, 4k context
    long chunk  Sq=512  pos=15872   chunked prefill, 16k context
Each shape prints one JSON line: device-event time per call of both paths,
their ratio, and the worst per-row relative error between them. The verify
line adds the achieved GB/s over the streamed cache bytes (K and V rows
0 .. pos+Sq-1 of the Hkv heads, once) next to attn_decode at the same
length: both are bound by that stream. Needs a GPU: a CPU timing says
nothing about the kernel.

A second JSON line per shape covers the paged cache
(K.attn_append_paged, the paged instantiation of ops/csrc/append.hip) on
the same rows held in a page pool: pages in order, pages randomly permuted, and the path the
paged engine took before that kernel existed (K.kv_page_gather of K and
of V, then K.attn_append on the copies), each next to the dense kernel.
All of them alternate within each of the three runs.
"""

import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))

H, HKV, B, D = 32, 8, 1, 128
PAGE = 64
SHAPES = [("verify", 5, 4096), ("chunk", 512, 3584),
          ("long chunk", 512, 15872)]


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


def _pool(torch, cache, table, num_pages):
    """Page pool [num_pages, Hkv, 64, 128] holding the rows of
    cache [1, Hkv, L, 128] at the pages table [pps] names (zeros
    elsewhere)."""
    hkv, L = cache.size(1), cache.size(2)
    pps = table.numel()
    padded = torch.zeros(hkv, pps * PAGE, D, device=cache.device,
                         dtype=cache.dtype)
    padded[:, :L] = cache[0]
    pool = torch.zeros(num_pages, hkv, PAGE, D, device=cache.device,
                       dtype=cache.dtype)
    pool[table.long()] = padded.view(hkv, pps, PAGE, D).permute(1, 0, 2, 3)
    return pool


def _paged_row(K, torch, name, Sq, pos, q, kc, vc, pos_t, scale, dense,
               args):
    """The paged kernel in both page orders and the gather + dense path
    on the same pools, against the dense kernel ``dense`` on the same
    rows."""
    L = pos + Sq
    pps = -(-L // PAGE)
    num_pages = pps + 8
    gen = torch.Generator().manual_seed(1)
    tables = {
        "in_order": torch.arange(pps, dtype=torch.int32),
        "permuted": torch.randperm(num_pages, generator=gen)[:pps].to(
            torch.int32),
    }
    fns = {"dense": dense}
    o_dense = dense()
    checks = {}
    for order, tbl in tables.items():
        tbl = tbl.to(q.device)
        kp = _pool(torch, kc, tbl, num_pages)
        vp = _pool(torch, vc, tbl, num_pages)
        tb = tbl.view(1, pps).contiguous()

        def paged(kp=kp, vp=vp, tb=tb):
            return K.attn_append_paged(q, kp, vp, tb, pos_t, scale,
                                       max_len=L)

        def gather(kp=kp, vp=vp, tb=tb):
            kg = K.kv_page_gather(kp, tb[0], L)
            vg = K.kv_page_gather(vp, tb[0], L)
            return K.attn_append(q, kg, vg, pos_t, scale, max_len=L)

        fns["paged_" + order] = paged
        fns["gather_" + order] = gather
        o = paged()
        assert torch.equal(gather(), o_dense), "gather path lost rows"
        d = (o.float() - o_dense.float()).norm(dim=-1) \
            / o_dense.float().norm(dim=-1)
        checks[order] = {"bit_equal_to_dense": bool(torch.equal(o, o_dense)),
                         "worst_row_rel_diff": float("%.3e" % d.max().item())}
    runs = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            runs[k].append(_time_ms(fn, args.warmup, args.iters))
    best = {k: min(v) for k, v in runs.items()}
    flops = 4.0 * B * H * Sq * D * (pos + (Sq + 1) / 2.0)
    res = {
        "metric": "attn_append_paged ms/call", "shape": name,
        "value": round(best["paged_in_order"], 4), "unit": "ms",
        "higher_is_better": False,
        "best_ms": {k: round(v, 4) for k, v in best.items()},
        "ms_runs": {k: [round(t, 4) for t in v] for k, v in runs.items()},
        "paged_over_dense": {
            o: round(best["paged_" + o] / best["dense"], 3) for o in tables},
        "gather_path_over_paged": {
            o: round(best["gather_" + o] / best["paged_" + o], 2)
            for o in tables},
        "tflops": {o: round(flops / (best["paged_" + o] * 1e9), 2)
                   for o in tables},
        "vs_dense": checks,
        "config": {"B": B, "H": H, "Hkv": HKV, "Sq": Sq, "pos": pos,
                   "pages": pps, "pool_pages": num_pages},
    }
    if name == "verify":
        stream_bytes = 2 * B * HKV * L * D * 2
        res["cache_stream_GBps"] = {
            o: round(stream_bytes / best["paged_" + o] / 1e6, 1)
            for o in tables}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    args = p.parse_args()

    import torch

    from metaflow_amd.ops import kernels as K

    if not torch.cuda.is_available():
        sys.exit("bench_append.py measures the GPU kernel: no GPU found")
    dev = torch.device("cuda", 0)
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(0)

    for name, Sq, pos in SHAPES:
        L = pos + Sq
        q = torch.randn(B, H, Sq, D, device=dev, dtype=torch.bfloat16)
        kc = torch.randn(B, HKV, L, D, device=dev, dtype=torch.bfloat16)
        vc = torch.randn(B, HKV, L, D, device=dev, dtype=torch.bfloat16)
        pos_t = torch.full((B,), pos, dtype=torch.int32, device=dev)

        def kern():
            return K.attn_append(q, kc, vc, pos_t, scale, max_len=L)

        def eager():
            return K.attn_append_ref(q, kc, vc, pos, scale)

        o, ref = kern().float(), eager().float()
        row_err = ((o - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
        # alternate the two paths so drift hits both alike
        t_k, t_e = [], []
        for _ in range(3):
            t_k.append(_time_ms(kern, args.warmup, args.iters))
            t_e.append(_time_ms(eager, args.warmup,
                                max(args.iters // 5, 5)))
        k_ms, e_ms = min(t_k), min(t_e)
        res = {
            "metric": "attn_append ms/call", "shape": name,
            "value": round(k_ms, 4), "unit": "ms",
            "higher_is_better": False,
            "eager_ms": round(e_ms, 4),
            "speedup_vs_eager": round(e_ms / k_ms, 2),
            "kernel_ms_runs": [round(t, 4) for t in t_k],
            "eager_ms_runs": [round(t, 4) for t in t_e],
            "worst_row_rel_err": float("%.3e" % row_err),
            "tflops": round(4.0 * B * H * Sq * D
                            * (pos + (Sq + 1) / 2.0) / (k_ms * 1e9), 2),
            "config": {"B": B, "H": H, "Hkv": HKV, "Sq": Sq, "pos": pos},
        }
        if name == "verify":
            stream_bytes = 2 * B * HKV * L * D * 2
            q1 = q[:, :, :1].contiguous()
            d_ms = min(_time_ms(
                lambda: K.attn_decode(q1, kc, vc, L, scale),
                args.warmup, args.iters) for _ in range(3))
            res["cache_stream_GBps"] = round(stream_bytes / k_ms / 1e6, 1)
            res["attn_decode_ms"] = round(d_ms, 4)
            res["attn_decode_GBps"] = round(stream_bytes / d_ms / 1e6, 1)
        print(json.dumps(res), flush=True)
        print(json.dumps(_paged_row(K, torch, name, Sq, pos, q, kc, vc,
                                    pos_t, scale, kern, args)), flush=True)
        del q, kc, vc


if __name__ == "__main__":
    main()
