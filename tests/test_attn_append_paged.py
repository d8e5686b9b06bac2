"""K.attn_append_paged off the GPU: the CPU reference path and the model
wiring (a later prefill chunk on a paged cache calls it, and no longer
gathers the prefix out of the pool)."""

import math

import torch

from metaflow_amd.models.llama import (KVCache, LlamaConfig,
                                       LlamaForCausalLM, PagedKVCache,
                                       PagedSlotView)
from metaflow_amd.ops import kernels as K

SCALE = 1.0 / math.sqrt(128)
PAGE = K.PAGE_ROWS


def test_cpu_reference_matches_append_ref_on_gathered_rows():
    """Shuffled page ownership, per-sequence pos, one pos = -1 sequence,
    NaN in every unowned page and in every row past pos + Sq: the CPU
    path equals attn_append_ref on the contiguous rows, bit for bit."""
    B, H, Hkv, Sq = 3, 4, 2, 5
    pos = [70, -1, 130]
    pps = 4
    g = torch.Generator().manual_seed(5)
    owned = sum(-(-(p + Sq) // PAGE) for p in pos if p >= 0)
    num_pages = owned + 3
    perm = torch.randperm(num_pages, generator=g).tolist()
    nan_page = perm.pop()
    q = torch.randn(B, H, Sq, 128, generator=g).to(torch.bfloat16)
    kp = torch.full((num_pages, Hkv, PAGE, 128), float("nan"),
                    dtype=torch.bfloat16)
    vp = torch.full_like(kp, float("nan"))
    table = torch.full((B, pps), nan_page, dtype=torch.int32)
    dense = []
    for b, p in enumerate(pos):
        if p < 0:
            dense.append(None)
            continue
        n = p + Sq
        k = torch.randn(1, Hkv, n, 128, generator=g).to(torch.bfloat16)
        v = torch.randn(1, Hkv, n, 128, generator=g).to(torch.bfloat16)
        dense.append((k, v))
        for j in range(-(-n // PAGE)):
            page = perm.pop()
            table[b, j] = page
            m = min(PAGE, n - j * PAGE)
            kp[page, :, :m] = k[0, :, j * PAGE:j * PAGE + m]
            vp[page, :, :m] = v[0, :, j * PAGE:j * PAGE + m]

    o = K.attn_append_paged(q, kp, vp, table, pos, SCALE)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    assert not torch.isnan(o.float()).any()
    for b, p in enumerate(pos):
        if p < 0:
            assert bool((o[b] == 0).all())
            continue
        k, v = dense[b]
        ref = K.attn_append_ref(q[b:b + 1], k, v, p, SCALE)
        assert not torch.isnan(ref.float()).any()
        assert torch.equal(o[b:b + 1], ref)
    # a tensor pos takes the same path
    o_t = K.attn_append_paged(q, kp, vp, table,
                              torch.tensor(pos, dtype=torch.int32), SCALE)
    assert torch.equal(o_t, o)


def test_later_chunk_on_paged_cache_calls_paged_append(monkeypatch):
    """40 tokens then 7 through a PagedSlotView: the second forward calls
    K.attn_append_paged once per layer with Sq == 7, never gathers, and
    gives the logits of the same two forwards on a dense KVCache."""
    torch.manual_seed(0)
    cfg = LlamaConfig.tiny(vocab=128, seq=256)
    model = LlamaForCausalLM(cfg).eval()
    appended, gathered = [], []
    real_append, real_gather = K.attn_append_paged, K.kv_page_gather
    in_append = [False]

    def counted_append(*a, **kw):
        appended.append(a[0].shape)
        in_append[0] = True
        try:
            return real_append(*a, **kw)
        finally:
            in_append[0] = False

    def counted_gather(*a, **kw):
        # the kernel's own CPU reference gathers by design; what must be
        # gone is the model's gather of the prefix
        if not in_append[0]:
            gathered.append(a[0].shape)
        return real_gather(*a, **kw)

    monkeypatch.setattr(K, "attn_append_paged", counted_append)
    monkeypatch.setattr(K, "kv_page_gather", counted_gather)
    g = torch.Generator().manual_seed(0)
    tokens = torch.randint(0, cfg.vocab_size, (1, 47), generator=g)
    with torch.no_grad():
        dense = KVCache(cfg, 1, 128, "cpu")
        ref_a = model(tokens[:, :40], cache=dense)
        ref_b = model(tokens[:, 40:], cache=dense)

        paged = PagedKVCache(cfg, 5, 2, 128, "cpu")
        assert paged.reserve(3)
        paged.ensure(0, 1)          # slot 1's page is not pool page 0
        paged.ensure(1, 47)
        paged.sync()
        view = PagedSlotView(paged, 1)
        out_a = model(tokens[:, :40], cache=view)
        assert appended == []       # the first chunk is the flash prefill
        out_b = model(tokens[:, 40:], cache=view)
    assert len(appended) == cfg.num_layers
    assert all(s[2] == 7 for s in appended)
    assert gathered == []
    assert view.pos == 47
    assert torch.equal(out_a, ref_a)
    assert torch.equal(out_b, ref_b)

