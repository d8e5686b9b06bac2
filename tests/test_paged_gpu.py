"""The paged KV cache on the GPU (paged.hip, and decode.hip's paged
instantiation): K.attn_decode_paged and K.kv_page_write against
CPU references, and the model / engine wiring on a paged cache.

The pool is larger than what the sequences own. Every unowned page and
every row past a sequence's length in its last page is NaN, table
entries past ceil(len/64) point at an all-NaN page, and owned pages are
handed out in shuffled order: a wrong read shows as a NaN in the output,
never as a fault. The check is PER ROW against fp32 attention_ref on rows
gathered on the CPU; 2e-2 is the project's kernel tolerance
(test_ops_gpu.py). The kernel is fp32 up to the bf16 store, so the worst
row sits at a few 1e-3.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 1.0 / math.sqrt(128)
TOL = 2e-2
PAGE = 64

# (B, H, Hkv, lengths, max_len)
DECODE_SHAPES = [
    # one row; exactly one full page; single split
    (2, 4, 2, [1, 64], 64),
    # one row into a new page; partial last page
    (2, 4, 2, [65, 200], 256),
    # inactive slot (output exactly 0); G = 4; split count from the
    # capacity: most splits are empty for the short sequence (the -inf
    # merge path), several non-empty ones for the long sequence
    (3, 8, 2, [0, 129, 1000], 2048),
]


def setup_module():
    from metaflow_amd.ops import kernels as K

    assert K.extension_loaded(), "_mfx_hip must be built for GPU tests"


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _paged_case(B, H, Hkv, lengths, max_len, seed):
    """CPU tensors: q, NaN-backed pools, the table, and each sequence's
    contiguous rows (the reference input)."""
    g = torch.Generator().manual_seed(seed)
    pps = -(-max_len // PAGE)
    owned = sum(-(-n // PAGE) for n in lengths)
    num_pages = owned + 4
    perm = torch.randperm(num_pages, generator=g).tolist()
    nan_page = perm.pop()
    q = torch.randn(B, H, 1, 128, generator=g).to(torch.bfloat16)
    kp = torch.full((num_pages, Hkv, PAGE, 128), float("nan"),
                    dtype=torch.bfloat16)
    vp = torch.full_like(kp, float("nan"))
    table = torch.full((B, pps), nan_page, dtype=torch.int32)
    rows = []
    for b, n in enumerate(lengths):
        k = torch.randn(Hkv, n, 128, generator=g).to(torch.bfloat16)
        v = torch.randn(Hkv, n, 128, generator=g).to(torch.bfloat16)
        rows.append((k, v))
        for j in range(-(-n // PAGE)):
            page = perm.pop()
            table[b, j] = page
            m = min(PAGE, n - j * PAGE)
            kp[page, :, :m] = k[:, j * PAGE:j * PAGE + m]
            vp[page, :, :m] = v[:, j * PAGE:j * PAGE + m]
    return q, kp, vp, table, rows


@pytest.mark.parametrize("B,H,Hkv,lengths,max_len", DECODE_SHAPES)
def test_attn_decode_paged_matches_reference(dev, B, H, Hkv, lengths,
                                             max_len):
    from metaflow_amd.ops import kernels as K

    q, kp, vp, table, rows = _paged_case(B, H, Hkv, lengths, max_len,
                                         seed=7)
    o = K.attn_decode_paged(q.to(dev), kp.to(dev), vp.to(dev),
                            table.to(dev), lengths, SCALE, max_len)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    o = o.float().cpu()
    worst = 0.0
    for b, n in enumerate(lengths):
        if n == 0:
            assert bool((o[b] == 0).all()), "inactive slot must be 0"
            continue
        k, v = rows[b]
        ref = K.attention_ref(q[b:b + 1].float(), k[None].float(),
                              v[None].float(), SCALE, causal=False)[0]
        assert not torch.isnan(ref).any()
        assert not torch.isnan(o[b]).any(), "read an unowned row"
        err = ((o[b] - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
        worst = max(worst, err)
    print("paged decode %s worst row rel err %.3e" % (lengths, worst))
    assert worst < TOL


# lengths of 512 at max_len 512: both launchers choose 2 splits, and the
# dense split of 256 rows is the paged split of 4 pages — same tile order.
# At 130 the dense kernel makes two 65-row splits, the paged one a 128-row
# and a 2-row split.
@pytest.mark.parametrize("lengths", [[512, 512], [512, 130]])
def test_attn_decode_paged_matches_dense_kernel(dev, lengths):
    """The dense decode kernel on the same rows, contiguous, with the same
    capacity and max_len: the two instantiations of one body. Gated at the
    kernel tolerance; bit equality is printed, not asserted."""
    from metaflow_amd.ops import kernels as K

    B, H, Hkv, max_len = 2, 4, 2, 512
    q, kp, vp, table, rows = _paged_case(B, H, Hkv, lengths, max_len,
                                         seed=13)
    Lmax = table.size(1) * PAGE
    kc = torch.full((B, Hkv, Lmax, 128), float("nan"), dtype=torch.bfloat16)
    vc = torch.full_like(kc, float("nan"))
    for b, (k, v) in enumerate(rows):
        kc[b, :, :k.size(1)] = k
        vc[b, :, :v.size(1)] = v
    gq = q.to(dev)
    o_p = K.attn_decode_paged(gq, kp.to(dev), vp.to(dev), table.to(dev),
                              lengths, SCALE, max_len)
    o_d = K.attn_decode_varlen(gq, kc.to(dev), vc.to(dev), lengths, SCALE,
                               max_len=max_len)
    torch.cuda.synchronize()
    print("paged vs dense decode %s bit-equal: %s"
          % (lengths, torch.equal(o_p, o_d)))
    o_p, o_d = o_p.float().cpu(), o_d.float().cpu()
    assert not torch.isnan(o_p).any() and not torch.isnan(o_d).any()
    err = ((o_p - o_d).norm(dim=-1) / o_d.norm(dim=-1)).max().item()
    print("paged vs dense decode %s worst per-row rel diff %.3e"
          % (lengths, err))
    assert err < TOL


@pytest.mark.parametrize("S,pos", [(1, [0, 63, -1]), (70, [0, 60, 130])])
def test_kv_page_write_bit_exact(dev, S, pos):
    from metaflow_amd.ops import kernels as K

    B, Hkv, num_pages, pps = 3, 2, 14, 4
    SENT = -7.0
    g = torch.Generator().manual_seed(11)
    perm = torch.randperm(num_pages, generator=g)[:B * pps]
    table = perm.view(B, pps).to(torch.int32)
    k = torch.randn(B, Hkv, S, 128, generator=g).to(torch.bfloat16)
    v = torch.randn(B, Hkv, S, 128, generator=g).to(torch.bfloat16)
    kp = torch.full((num_pages, Hkv, PAGE, 128), SENT, dtype=torch.bfloat16)
    want_k, want_v = kp.clone(), kp.clone()
    for b, p in enumerate(pos):
        if p < 0:
            continue
        for s in range(S):
            page, r = int(table[b, (p + s) // PAGE]), (p + s) % PAGE
            want_k[page, :, r] = k[b, :, s]
            want_v[page, :, r] = v[b, :, s]
    kp_d, vp_d = kp.to(dev), kp.to(dev)
    # a strided source (the decode step's V is a slice of the QKV GEMM
    # output): same values, rows 256 elements apart
    wide = torch.zeros(B, Hkv, S, 256, dtype=torch.bfloat16, device=dev)
    wide[..., 128:] = v.to(dev)
    K.kv_page_write(k.to(dev), wide[..., 128:], kp_d, vp_d, table.to(dev),
                    torch.tensor(pos, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    # bit-equal rows, sentinel everywhere else (pos = -1 wrote nothing)
    assert torch.equal(kp_d.cpu().view(torch.int16),
                       want_k.view(torch.int16))
    assert torch.equal(vp_d.cpu().view(torch.int16),
                       want_v.view(torch.int16))


@pytest.fixture(scope="module")
def tiny_llama():
    from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    return LlamaForCausalLM(
        LlamaConfig.tiny(vocab=128, seq=256)).to("cuda:0").eval()


def test_decode_step_paged_matches_dense(dev, tiny_llama):
    """One batched decode step on a paged cache and on a KVCache holding
    the same rows. Logits, not tokens: the two kernels split the range
    differently."""
    from metaflow_amd.models.llama import KVCache, PagedKVCache
    from metaflow_amd.ops import kernels as K

    m = tiny_llama
    cfg = m.cfg
    positions = [5, 64, 130]
    B = len(positions)
    torch.manual_seed(3)
    dense = KVCache(cfg, B, 256, dev)
    paged = PagedKVCache(cfg, 9, B, 256, dev)
    assert paged.reserve(9)
    # hand the pages out interleaved, so no slot's pages are contiguous
    for rows in (1, 65, 129):
        for b, p in enumerate(positions):
            paged.ensure(b, min(rows, p + 1))
    paged.sync()
    for li in range(cfg.num_layers):
        dense.k[li].normal_()
        dense.v[li].normal_()
        paged.k_pages[li].fill_(float("nan"))
        paged.v_pages[li].fill_(float("nan"))
        for b, p in enumerate(positions):
            K.kv_page_write(dense.k[li][b:b + 1, :, :p],
                            dense.v[li][b:b + 1, :, :p],
                            paged.k_pages[li], paged.v_pages[li],
                            paged.block_table[b:b + 1], [0])
    tokens = torch.tensor([[3], [9], [27]], device=dev)
    ref = m.decode_step(tokens, dense, positions).float()
    out = m.decode_step(tokens, paged, positions).float()
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    err = ((out - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()
    print("paged vs dense decode_step logits rel err %.3e" % err)
    assert err < TOL
    # the step wrote each slot's new row where the dense step did
    for b, p in enumerate(positions):
        got = K.kv_page_gather(paged.k_pages[0], paged.block_table[b],
                               p + 1)
        assert torch.equal(got[0, :, p], dense.k[0][b, :, p])


# four requests that cross page boundaries: in decode (60 + 10), in the
# prompt (70), exactly at one (64 + 1) and a short one
GRAPH_REQUESTS = [
    ([(3 * i + 1) % 128 for i in range(60)], 10),
    ([(5 * i + 2) % 128 for i in range(70)], 6),
    ([(7 * i + 3) % 128 for i in range(64)], 3),
    ([9, 4, 77], 5),
]


def test_paged_engine_graph_matches_eager(dev, tiny_llama):
    from metaflow_amd.serving import ContinuousBatcher

    outs = []
    for graph in (True, False):
        b = ContinuousBatcher(tiny_llama, max_batch=3, max_len=128,
                              graph=graph, num_pages=5)
        assert (b._graph is not None) == graph
        reqs = [b.submit(p, n) for p, n in GRAPH_REQUESTS]
        res = b.run()
        outs.append([res[r.id] for r in reqs])
        assert b.cache.free_pages == 5
        assert bool((b.cache.table_host == -1).all())
    for toks, (_p, n) in zip(outs[0], GRAPH_REQUESTS):
        assert len(toks) == n
    # both launch the same grids: greedy tokens are identical
    assert outs[0] == outs[1]


def test_paged_engine_mixtral_runs_eager(dev):
    from metaflow_amd.models.mixtral import (MixtralConfig,
                                             MixtralForCausalLM)
    from metaflow_amd.serving import ContinuousBatcher

    torch.manual_seed(0)
    m = MixtralForCausalLM(
        MixtralConfig.tiny(vocab=128, seq=256)).to(dev).eval()
    b = ContinuousBatcher(m, max_batch=2, max_len=128, num_pages=4,
                          prefill_chunk=32)
    assert b._graph is None
    reqs = [b.submit(p, n) for p, n in GRAPH_REQUESTS[:3]]
    res = b.run()
    for r, (_p, n) in zip(reqs, GRAPH_REQUESTS):
        assert r.done and len(res[r.id]) == n
        assert all(0 <= t < 128 for t in res[r.id])
    assert b.cache.free_pages == 4
