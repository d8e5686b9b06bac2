#!/usr/bin/env python3
"""Flagship benchmark: @parallel Llama-3-8B bf16 train step (BASELINE
config 3) — tokens/sec, whole-job aggregate.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]
                    [--full]

A plain run sets up, warms up, times exactly K steps and prints one JSON
result line (ms_per_step = wall milliseconds per timed step). With
--dump-outputs it first writes the last timed step's results as .npy
files; seeds are fixed, so the same arguments give the same inputs on
every run. --full is reserved for secondary measurements (none today).

For N>1 the driver launches this under torch.distributed.run (one rank per
GPU, RCCL over xGMI); this script is exactly the body the @parallel gang
step runs inside the workflow engine (see tests/flows/train_flow.py for the
FlowSpec-wrapped version). Synthetic data (random tokens), random-init
weights, bf16 compute, fp32 Adam moments.
"""

import argparse
import json
import os
import time

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--batch", type=int, default=8,
                   help="per-GPU micro batch")
    p.add_argument("--seq", type=int, default=4096)
    p.add_argument("--model", type=str, default="llama3-8b",
                   choices=["llama3-8b", "llama3-70b", "tiny",
                            "mixtral-8x7b", "mixtral-2x7b",
                            "mixtral-tiny"])
    p.add_argument("--bucket-mb", type=int, default=64)
    p.add_argument("--cp", action="store_true",
                   help="context parallelism: all ranks form one ring-"
                        "attention group over a single shared batch "
                        "(seq sharded across ranks)")
    p.add_argument("--tp", action="store_true",
                   help="tensor parallelism: all ranks form one "
                        "Megatron-style shard group over a single "
                        "shared batch")
    p.add_argument("--lr", type=float, default=3e-4)
    p.add_argument("--recompute", action="store_true",
                   help="checkpoint decoder-layer activations "
                        "(recompute in backward): O(1)-layer activation "
                        "memory for 70B/long-seq configs")
    p.add_argument("--zero", action="store_true",
                   help="ZeRO-1: shard optimizer state (fp32 m/v) and "
                        "grad ownership across DP ranks — the memory "
                        "mode that fits llama3-70b on 8x288 GB")
    p.add_argument("--fp8", action="store_true",
                   help="decoder projections' forward GEMMs in OCP E4M3 "
                        "(delayed scaling, bf16 backward) — reported "
                        "honestly as dtype fp8-e4m3-fwd, NOT the bf16 "
                        "headline")
    p.add_argument("--fp8-bwd", action="store_true",
                   help="with --fp8: dgrad/wgrad GEMMs in E4M3 too "
                        "(delayed-scaled dy) — dtype fp8-e4m3-fwd-bwd")
    p.add_argument("--tunableop", action="store_true",
                   help="enable PyTorch TunableOp (hipBLASLt algorithm "
                        "autotuning) during warmup")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step produced (loss, plus a fixed seeded sample "
                        "of the updated parameters and of the gradients) "
                        "as DIR/<name>.npy in float32")
    p.add_argument("--full", action="store_true",
                   help="also run every secondary measurement or check "
                        "(none today: a plain run already does only "
                        "what the headline figure needs — this is "
                        "where any future extra belongs)")
    return p.parse_args()


# elements sampled from each flat buffer by --dump-outputs (float32:
# 8 MB per array, far below the 64 MB a dump may take in all)
DUMP_SAMPLE = 1 << 21
DUMP_SEED = 20240229


def dump_outputs(out_dir, flat, step_losses):
    """Write the last timed step's results as float32 .npy files.

    loss.npy         [1]  loss returned by the last timed step
    step_losses.npy  [K]  loss of every timed step, in order
    params.npy       [n]  updated bf16 parameters (flat buffer sample)
    grads.npy        [n]  gradients the optimizer consumed (same indices)

    Buffers larger than DUMP_SAMPLE are sampled at indices drawn once
    from a fixed seed, so two builds run with the same arguments dump
    the same elements. Alignment padding between parameters is never
    initialised and is left out.
    """
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    offsets = np.asarray(flat.offsets, dtype=np.int64)
    numels = np.asarray([p.numel() for p in flat.params], dtype=np.int64)
    if flat.total <= DUMP_SAMPLE:
        idx = np.arange(flat.total, dtype=np.int64)
    else:
        rng = np.random.RandomState(DUMP_SEED)
        idx = np.sort(rng.randint(0, flat.total, size=DUMP_SAMPLE,
                                  dtype=np.int64))
    owner = np.searchsorted(offsets, idx, side="right") - 1
    idx = idx[idx - offsets[owner] < numels[owner]]  # drop padding
    sel = torch.from_numpy(idx).to(flat.flat_param.device)
    arrays = {
        "loss": step_losses[-1:].float(),
        "step_losses": step_losses.float(),
        "params": flat.flat_param.index_select(0, sel).float(),
        "grads": flat.flat_grad.index_select(0, sel).float(),
    }
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"),
                t.detach().cpu().numpy().astype(np.float32))


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = args.gpus if world == 1 else world

    import torch.distributed as dist

    from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from metaflow_amd.parallel.ddp import (
        FlatParamModel,
        FusedAdamW,
        init_process_group_from_env,
    )

    if args.tunableop:
        os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
        os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "1")
        os.environ.setdefault("PYTORCH_TUNABLEOP_MAX_TUNING_DURATION_MS",
                              "100")
        os.environ.setdefault(
            "PYTORCH_TUNABLEOP_MAX_TUNING_ITERATIONS", "30")
        os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME",
                              "/tmp/mfx_tunableop_%d.csv" % rank)

    use_gpu = torch.cuda.is_available()
    device = torch.device("cuda", local_rank) if use_gpu else \
        torch.device("cpu")
    if use_gpu:
        torch.cuda.set_device(device)

    distributed = world > 1
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        init_process_group_from_env()

    from metaflow_amd.models.mixtral import (
        MixtralConfig,
        MixtralForCausalLM,
    )

    model_factories = {
        "llama3-8b": (LlamaConfig.llama3_8b, LlamaForCausalLM),
        "llama3-70b": (LlamaConfig.llama3_70b, LlamaForCausalLM),
        "tiny": (LlamaConfig.tiny, LlamaForCausalLM),
        "mixtral-8x7b": (MixtralConfig.mixtral_8x7b, MixtralForCausalLM),
        "mixtral-2x7b": (MixtralConfig.mixtral_2x7b, MixtralForCausalLM),
        "mixtral-tiny": (MixtralConfig.tiny, MixtralForCausalLM),
    }
    cfg_fn, model_cls = model_factories[args.model]
    cfg = cfg_fn()
    if args.fp8_bwd:
        args.fp8 = True
    if args.fp8:
        assert args.model in ("llama3-8b", "llama3-70b", "tiny"), \
            "--fp8 supports the Llama family"
        cfg.fp8 = True
        cfg.fp8_bwd = args.fp8_bwd
    if args.recompute:
        cfg.recompute = True
    seq = min(args.seq, cfg.max_seq_len)

    use_tp = args.tp and distributed
    use_cp = args.cp and distributed and not use_tp
    if use_tp:
        assert args.model in ("llama3-8b", "llama3-70b", "tiny"), \
            "--tp supports the Llama family"
        if cfg.num_kv_heads % world:
            # tiny config: widen the GQA group so heads shard evenly
            cfg.num_heads = max(cfg.num_heads, 2 * world)
            cfg.num_kv_heads = world
    if use_cp:
        assert args.model in ("llama3-8b", "llama3-70b", "tiny"), \
            "--cp supports the Llama family"
        assert seq % world == 0, "--cp needs seq %% world == 0"
        if use_gpu:
            assert (seq // world) % 256 == 0, \
                "--cp on GPU needs per-rank seq %% 256 == 0"

    torch.manual_seed(1234)  # same init on all ranks (DP)
    t0 = time.time()
    with torch.device(device):  # construct + random-init directly on GPU
        if use_tp:
            from metaflow_amd.models.llama_tp import TPLlamaForCausalLM

            model = TPLlamaForCausalLM(cfg, dist.group.WORLD)
        elif use_cp:
            model = model_cls(cfg, cp_group=dist.group.WORLD)
        else:
            model = model_cls(cfg)
    dp_group = None
    if use_tp:
        # tp spans the whole job: each rank is its own dp group (shards
        # must never be averaged across tp ranks)
        for r in range(world):
            g = dist.new_group([r])
            if r == rank:
                dp_group = g
    flat = FlatParamModel(model, bucket_mb=args.bucket_mb,
                          group=dp_group, zero=args.zero)
    flat.install_overlap_hooks()
    opt = FusedAdamW(flat, lr=args.lr)
    if rank == 0:
        print("# model %s: %.2fB params, init %.1fs"
              % (args.model, model.num_params() / 1e9, time.time() - t0),
              flush=True)

    # synthetic batch (fixed per rank but distinct across ranks: loss must
    # fall, proving a real fwd+bwd+optimizer step is in the timed region).
    # Under --cp every rank sees the SAME batch and takes its seq shard.
    torch.manual_seed(5678 + (0 if (use_cp or use_tp) else rank))
    tokens = torch.randint(0, cfg.vocab_size, (args.batch, seq + 1),
                           device=device)
    inp, tgt = tokens[:, :-1], tokens[:, 1:].contiguous()
    if use_cp:
        sc = seq // world
        sl = slice(rank * sc, (rank + 1) * sc)
        inp = inp[:, sl].contiguous()
        tgt = tgt[:, sl].contiguous()

    comm_ms = []

    def one_step():
        flat.zero_grad()
        loss = model(inp, tgt)
        loss.backward()
        flat.finish_grad_sync()
        comm_ms.append(getattr(flat, "last_comm_wait_ms", 0.0))
        opt.step()
        return loss

    losses = []
    for _ in range(args.warmup):
        losses.append(one_step())

    if distributed:
        dist.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    t_start = time.time()
    for _ in range(args.steps):
        losses.append(one_step())
    if use_gpu:
        torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    elapsed = time.time() - t_start

    # max over ranks
    if distributed:
        t = torch.tensor([elapsed], device=device if use_gpu else "cpu",
                         dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    first_loss = float(losses[0].item())
    last_loss = float(losses[-1].item())

    # cp/tp: one shared batch across the group; dp: one batch per rank
    shared = use_cp or use_tp
    tokens_per_step = args.batch * seq * (1 if shared else n_gpus)
    toks_per_sec = tokens_per_step * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if rank == 0:
        out = {
            "metric": "tokens/sec",
            "value": toks_per_sec,
            "unit": "tokens/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong" if shared else "weak",
            "vs_baseline": None,
            "dtype": ("fp8-e4m3-fwd-bwd" if args.fp8_bwd else
                      "fp8-e4m3-fwd") if args.fp8 else "bf16",
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": args.batch * (1 if shared else n_gpus),
                "seq_len": seq,
                "parallelism": ("tp%d" % n_gpus if use_tp else
                                ("cp%d" if use_cp else
                                 ("dp%d-zero1" if args.zero else "dp%d"))
                                % n_gpus),
                "first_loss": round(first_loss, 4),
                "last_loss": round(last_loss, 4),
                # NON-hidden gradient-comm wait per timed step (rank 0):
                # the number that explains the 1/2/4/8 scaling curve
                "comm_wait_ms": round(
                    sum(comm_ms[args.warmup:])
                    / max(1, len(comm_ms) - args.warmup), 2),
            },
        }
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, flat, torch.stack(
                [l.detach().reshape(()) for l in losses[args.warmup:]]))
        print(json.dumps(out), flush=True)

    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
