"""The sampling loop shared by the models' ``generate``."""

import torch

from .kv_cache import KVCache


@torch.no_grad()
def generate(model, tokens, max_new_tokens, temperature=0.0, top_k=None):
    """Autoregressive decode with a KV cache: flash-kernel prefill, cached
    attention for the one-token decode steps. temperature=0 is greedy."""
    B, S0 = tokens.shape
    cache = KVCache(model.cfg, B, S0 + max_new_tokens, tokens.device,
                    dtype=model.embed.weight.dtype)
    out = tokens
    logits = model.forward(tokens, cache=cache)
    for _ in range(max_new_tokens):
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
