"""The sampling loop shared by the models' ``generate``."""

import torch

from ..ops import kernels as K
from .kv_cache import KVCache


def fresh_seed():
    """A seed taken from torch's default CPU generator, so that
    torch.manual_seed governs what follows from it."""
    return int(torch.randint(0, 2 ** 62, ()))


def seeded_generator(seed=None):
    """A CPU generator for one sequence's draws; ``None`` = fresh_seed()."""
    if seed is None:
        seed = fresh_seed()
    g = torch.Generator()
    g.manual_seed(int(seed))
    return g


def draw(gen):
    """The generator's next fp32 uniform in [0, 1): one per new token."""
    return float(torch.rand((), generator=gen, dtype=torch.float32))


@torch.no_grad()
def generate(model, tokens, max_new_tokens, temperature=0.0, top_k=None,
             top_p=None, seed=None):
    """Autoregressive decode with a KV cache: flash-kernel prefill, cached
    attention for the one-token decode steps. temperature=0 is greedy.

    With ``top_p`` and ``seed`` both None, sampling is a top-k mask and a
    torch.multinomial on the global RNG. Giving either selects the fused
    sampler (ops/kernels.py sample_tokens) with per-row generators: row b
    draws from a CPU generator seeded ``seed + b`` (``seed=None`` takes
    one from the default generator), one fp32 uniform per new token —
    the draws and the selection rule of a serving-engine request with
    the same parameters and seed ``seed + b``."""
    B, S0 = tokens.shape
    cache = KVCache(model.cfg, B, S0 + max_new_tokens, tokens.device,
                    dtype=model.embed.weight.dtype)
    out = tokens
    logits = model.forward(tokens, cache=cache)
    fused = top_p is not None or seed is not None
    if fused:
        if seed is None:
            seed = fresh_seed()
        gens = [seeded_generator(seed + b) for b in range(B)]
        dev = tokens.device
        sampled = bool(temperature and temperature > 0)
        temp_t = torch.full((B,), float(temperature) if sampled else 0.0,
                            dtype=torch.float32, device=dev)
        topk_t = torch.full((B,), int(top_k or 0), dtype=torch.int32,
                            device=dev)
        topp_t = torch.full((B,), 1.0 if top_p is None else float(top_p),
                            dtype=torch.float32, device=dev)
    for _ in range(max_new_tokens):
        if fused:
            u = torch.tensor([draw(g) if sampled else 0.0 for g in gens],
                             dtype=torch.float32, device=dev)
            nxt = K.sample_tokens(logits[:, -1], temp_t, topk_t, topp_t,
                                  u)[:, None]
            out = torch.cat([out, nxt], dim=1)
            logits = model.forward(nxt, cache=cache)
            continue
        last = logits[:, -1].float()
        if temperature and temperature > 0:
            last = last / temperature
            if top_k:
                kth = torch.topk(last, top_k, dim=-1).values[:, -1:]
                last = last.masked_fill(last < kth, float("-inf"))
            probs = torch.softmax(last, dim=-1)
            nxt = torch.multinomial(probs, 1)
        else:
            nxt = last.argmax(dim=-1, keepdim=True)
        out = torch.cat([out, nxt], dim=1)
        logits = model.forward(nxt, cache=cache)
    return out
