"""Paged KV cache on the CPU reference paths: the page allocator, the
paged decode / page-write references against their contiguous
counterparts, and the paged serving engine against the dense one."""

import pytest
import torch

from metaflow_amd.models.llama import (KVCache, LlamaConfig,
                                       LlamaForCausalLM, PagedKVCache)
from metaflow_amd.ops import kernels as K
from metaflow_amd.serving import ContinuousBatcher

PAGE = 64


@pytest.fixture(scope="module")
def tiny_llama():
    torch.manual_seed(0)
    return LlamaForCausalLM(LlamaConfig.tiny(vocab=128, seq=256)).eval()


@pytest.fixture(scope="module")
def tiny_mixtral():
    from metaflow_amd.models.mixtral import (MixtralConfig,
                                             MixtralForCausalLM)

    torch.manual_seed(0)
    return MixtralForCausalLM(MixtralConfig.tiny(vocab=128, seq=256)).eval()


def _cache(num_pages=6, max_batch=3, max_len=256):
    return PagedKVCache(LlamaConfig.tiny(), num_pages, max_batch, max_len,
                        "cpu")


# ------------------------------------------------------------- allocator
def test_page_constant_matches_kernel_layout():
    assert K.PAGE_ROWS == PAGE and PagedKVCache.PAGE == PAGE
    c = _cache()
    assert c.k_pages[0].shape == (6, 1, PAGE, 128)
    assert c.table_host.shape == (3, 4) and c.table_host.dtype == torch.int32
    assert bool((c.table_host == -1).all())
    assert c.free_pages == 6


def test_ensure_across_boundary_allocates_one_page():
    c = _cache()
    assert c.reserve(3)
    c.ensure(0, 1)
    assert c.free_pages == 5
    c.ensure(0, PAGE)          # still the first page
    assert c.free_pages == 5
    c.ensure(0, PAGE + 1)      # first row of the second page
    assert c.free_pages == 4
    c.ensure(0, 2 * PAGE)
    assert c.free_pages == 4
    row = c.table_host[0].tolist()
    assert row[0] >= 0 and row[1] >= 0 and row[0] != row[1]
    assert row[2:] == [-1, -1]
    assert bool((c.table_host[1:] == -1).all())


def test_free_slot_returns_pages_and_resets_entries():
    c = _cache()
    assert c.reserve(4)
    c.ensure(0, 130)           # 3 pages
    c.ensure(1, 10)            # 1 page
    owned0 = c.table_host[0, :3].tolist()
    assert c.free_pages == 2
    c.free_slot(0)
    assert c.free_pages == 5
    assert bool((c.table_host[0] == -1).all())
    assert int(c.table_host[1, 0]) >= 0
    # LIFO: the pages just freed are the next ones handed out
    c.ensure(2, 1)
    assert int(c.table_host[2, 0]) in owned0


def test_reserve_fails_when_exhausted_and_recovers():
    c = _cache(num_pages=6)
    assert c.reserve(4)
    assert not c.reserve(3)    # 4 + 3 > 6
    assert c.reserve(2)
    assert not c.reserve(1)
    c.release_reservation(4)
    assert c.reserve(3)
    with pytest.raises(AssertionError):
        c.release_reservation(6)   # only 5 are reserved


def test_double_free_raises():
    c = _cache()
    assert c.reserve(1)
    c.ensure(0, 5)
    c.free_slot(0)
    with pytest.raises(AssertionError):
        c.free_slot(0)


def test_allocation_beyond_reservation_raises():
    c = _cache()
    assert c.reserve(1)
    c.ensure(0, PAGE)
    with pytest.raises(AssertionError):
        c.ensure(0, PAGE + 1)


def test_sync_copies_only_when_changed():
    c = _cache()
    assert c.reserve(2)
    c.ensure(1, 100)
    assert not torch.equal(c.block_table, c.table_host)
    c.sync()
    assert torch.equal(c.block_table, c.table_host)
    assert c.block_table.dtype == torch.int32
    # no change since: sync() must not copy (a marker survives it)
    c.block_table[2, 3] = 77
    c.sync()
    assert int(c.block_table[2, 3]) == 77
    c.free_slot(1)
    c.sync()
    assert torch.equal(c.block_table, c.table_host)
    assert bool((c.block_table == -1).all())


# ------------------------------------------------------ kernel references
def _paged_copy(kc, vc, lengths, num_pages, seed):
    """Scatter contiguous caches [B, Hkv, Lmax, 128] into a shuffled
    pool; returns (k_pages, v_pages, table)."""
    B, Hkv, Lmax, D = kc.shape
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(num_pages, generator=g).tolist()
    kp = torch.full((num_pages, Hkv, PAGE, D), float("nan"),
                    dtype=kc.dtype)
    vp = torch.full_like(kp, float("nan"))
    table = torch.full((B, -(-Lmax // PAGE)), -1, dtype=torch.int32)
    for b in range(B):
        for j in range(-(-lengths[b] // PAGE)):
            page = perm.pop()
            table[b, j] = page
            n = min(PAGE, lengths[b] - j * PAGE)
            kp[page, :, :n] = kc[b, :, j * PAGE:j * PAGE + n]
            vp[page, :, :n] = vc[b, :, j * PAGE:j * PAGE + n]
    return kp, vp, table


def test_attn_decode_paged_ref_matches_varlen_exactly():
    torch.manual_seed(0)
    B, H, Hkv, Lmax = 3, 4, 2, 200
    lengths = [0, 65, 200]
    q = torch.randn(B, H, 1, 128, dtype=torch.bfloat16)
    kc = torch.randn(B, Hkv, Lmax, 128, dtype=torch.bfloat16)
    vc = torch.randn_like(kc)
    kp, vp, table = _paged_copy(kc, vc, lengths, 9, seed=1)
    ref = K.attn_decode_varlen(q, kc, vc, lengths, 0.0883)
    o = K.attn_decode_paged(q, kp, vp, table, lengths, 0.0883, Lmax)
    assert not torch.isnan(ref).any()
    assert torch.equal(o, ref)
    assert bool((o[0] == 0).all())
    # the gather is the contiguous prefix
    g = K.kv_page_gather(kp, table[2], 200)
    assert g.shape == (1, Hkv, 200, 128) and g.is_contiguous()
    assert torch.equal(g[0], kc[2])


def test_kv_page_write_ref_matches_slice_assignment():
    torch.manual_seed(0)
    B, Hkv, Lmax, num_pages = 3, 2, 256, 12
    table = torch.tensor([[3, 7, 0, 9], [5, 1, 11, 2], [4, 6, 8, 10]],
                         dtype=torch.int32)
    for S, pos in ((1, [0, 63, -1]), (70, [0, 60, 130])):
        kp = torch.full((num_pages, Hkv, PAGE, 128), -7.0,
                        dtype=torch.bfloat16)
        vp = torch.full_like(kp, -7.0)
        kc = torch.full((B, Hkv, Lmax, 128), -7.0, dtype=torch.bfloat16)
        vc = torch.full_like(kc, -7.0)
        k = torch.randn(B, Hkv, S, 128, dtype=torch.bfloat16)
        v = torch.randn_like(k)
        K.kv_page_write(k, v, kp, vp, table, pos)
        for b, p in enumerate(pos):
            if p >= 0:
                kc[b, :, p:p + S] = k[b]
                vc[b, :, p:p + S] = v[b]
        for b in range(B):
            assert torch.equal(K.kv_page_gather(kp, table[b], Lmax)[0],
                               kc[b])
            assert torch.equal(K.kv_page_gather(vp, table[b], Lmax)[0],
                               vc[b])


def test_decode_step_paged_matches_dense_cpu(tiny_llama):
    """One batched decode step: same cached rows in both layouts, one
    slot taking no part (-1) in the paged step."""
    m = tiny_llama
    cfg = m.cfg
    torch.manual_seed(3)
    positions = [5, 64, 130]
    dense = KVCache(cfg, 4, 256, "cpu")
    paged = PagedKVCache(cfg, 8, 4, 256, "cpu")
    assert paged.reserve(8)
    for li in range(cfg.num_layers):
        dense.k[li].normal_()
        dense.v[li].normal_()
    for b, p in enumerate(positions):
        paged.ensure(b, p + 1)
    paged.sync()
    for li in range(cfg.num_layers):
        for b, p in enumerate(positions):
            K.kv_page_write(dense.k[li][b:b + 1, :, :p],
                            dense.v[li][b:b + 1, :, :p],
                            paged.k_pages[li], paged.v_pages[li],
                            paged.block_table[b:b + 1], [0])
    tokens = torch.tensor([[3], [9], [27], [0]])
    ref = m.decode_step(tokens, dense, positions + [0])
    out = m.decode_step(tokens, paged, positions + [-1])
    assert torch.equal(out[:3], ref[:3])
    assert not torch.isnan(out).any()


# ----------------------------------------------------------------- engine
# test_serving.test_continuous_batching_token_exact's request set, plus
# one request whose decode crosses a page boundary (60 + 10 > 64)
REQUESTS = [
    ([5, 9, 17, 4], 6),
    (list(range(2, 30)), 5),
    ([100, 101], 8),
    ([7] * 11, 4),
    ([64, 3, 99, 12, 54, 23], 7),
    ([(3 * i + 1) % 128 for i in range(60)], 10),
]


def _run(model, requests, **kw):
    b = ContinuousBatcher(model, **kw)
    reqs = [b.submit(p, n) for p, n in requests]
    out = b.run()
    assert all(r.done for r in reqs)
    return b, [out[r.id] for r in reqs]


def _assert_drained(b):
    assert b.cache.free_pages == b.cache.num_pages
    assert bool((b.cache.table_host == -1).all())
    assert b.cache.reserve(b.cache.num_pages)   # nothing left reserved
    b.cache.release_reservation(b.cache.num_pages)


@pytest.mark.parametrize("chunk", [None, 16])
@pytest.mark.parametrize("family", ["llama", "mixtral"])
def test_paged_engine_token_exact(family, chunk, tiny_llama, tiny_mixtral):
    model = tiny_llama if family == "llama" else tiny_mixtral
    _, ref = _run(model, REQUESTS, max_batch=2, max_len=128,
                  prefill_chunk=chunk)
    b, out = _run(model, REQUESTS, max_batch=2, max_len=128,
                  prefill_chunk=chunk, num_pages=4)
    assert out == ref
    for toks, (_p, n) in zip(out, REQUESTS):
        assert len(toks) == n
    _assert_drained(b)


def test_unpaged_engine_untouched(tiny_llama):
    b = ContinuousBatcher(tiny_llama, max_batch=2, max_len=64)
    assert isinstance(b.cache, KVCache) and not b.paged


def test_small_pool_serves_more_than_dense_slots_could(tiny_llama):
    """max_batch=4 x max_len=256 dense slots would need 16 pages; 6
    suffice for short requests, several of them active at once."""
    requests = [([3 + i, 7, 11, 2 * i + 1], 4 + (i % 3)) for i in range(8)]
    _, ref = _run(tiny_llama, requests, max_batch=4, max_len=256)
    b = ContinuousBatcher(tiny_llama, max_batch=4, max_len=256,
                          num_pages=6)
    reqs = [b.submit(p, n) for p, n in requests]
    most_active = 0
    while b.queue or any(r is not None for r in b.slots):
        most_active = max(most_active, b.step())
        assert b.cache.free_pages >= 0
    assert [r.generated for r in reqs] == ref
    assert most_active > 1
    _assert_drained(b)


def test_reservation_that_does_not_fit_waits_for_a_release(tiny_llama):
    """FIFO admission: the 4-page request cannot join the 2-page one in a
    5-page pool until that one finishes; the short request queued behind
    it does not overtake."""
    big = ([9] * 200, 20)        # ceil(220 / 64) = 4 pages
    first = ([5] * 100, 3)       # 2 pages
    last = ([4, 8], 2)           # 1 page, would fit at once
    _, ref = _run(tiny_llama, [first, big, last], max_batch=4, max_len=256)
    b = ContinuousBatcher(tiny_llama, max_batch=4, max_len=256,
                          num_pages=5)
    r_first, r_big, r_last = [b.submit(p, n) for p, n in (first, big, last)]
    b.step()
    assert b.slots.count(None) == 3          # slots are free ...
    assert list(b.queue) == [r_big, r_last]  # ... the head still waits
    assert not r_last.generated              # and nobody overtook it
    while not r_first.done:
        assert r_big in b.queue
        b.step()
    b.step()
    assert r_big not in b.queue and r_big.generated
    b.run()
    assert [r_first.generated, r_big.generated, r_last.generated] == ref
    _assert_drained(b)


def test_request_that_can_never_fit_fails(tiny_llama):
    b = ContinuousBatcher(tiny_llama, max_batch=2, max_len=256, num_pages=2)
    b.submit([1] * 100, 60)      # 3 pages > pool
    with pytest.raises(AssertionError):
        b.step()
    b2 = ContinuousBatcher(tiny_llama, max_batch=2, max_len=64, num_pages=8)
    b2.submit([1] * 60, 10)      # longer than the slot capacity
    with pytest.raises(AssertionError):
        b2.step()
