"""append_fp8.hip on the GPU: K.attn_append_paged_fp8 per row against fp32
attn_append_ref on the requantised rows, at the kernel tolerance 2e-2 (TOL
of the FP8 decode and the paged append tests). Cases as in
test_decode_fp8_gpu.py: row magnitudes over 2^+-6, a pool larger than what
is owned holding byte 0x7F with NaN scales, shuffled pages, a spare table
column pointing at a NaN page, one all-zero K row inside the visible range.
Worst row measured on an MI355X: docs/KERNELS.md, "FP8 paged append"."""

import math

import pytest
import torch

from metaflow_amd.ops import kernels as K

from .test_attn_append_paged_gpu import _check_rows, _reference
from .test_decode_fp8_gpu import _requant, _spread_rows

pytestmark = pytest.mark.gpu

SCALE = 1.0 / math.sqrt(128)
TOL = 2e-2
PAGE = 64

# (B, H, Hkv, Sq, pos, max_len)
SHAPES = [
    (2, 4, 2, 5, [300, 0], None),       # 1-wave, partial last page, pos 0
    (2, 8, 2, 130, [0, 191], None),     # 4-wave, prefetch, 2 live rows, G=4
    (1, 2, 1, 64, [64], None),          # pos on a page boundary
    (1, 2, 1, 128, [3], 2048),          # splits from the capacity
    (1, 2, 1, 64, [1000], 2048),        # several live splits, the merge
    (1, 32, 1, 5, [130], None),         # G = 32
]


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _fp8_case(B, H, Hkv, Sq, pos, max_len, seed, num_pages=None):
    """CPU: q, (pools, scales) NaN-backed, the table with one spare column,
    and per participating sequence the requantised fp32 rows."""
    g = torch.Generator().manual_seed(seed)
    cap = max_len if max_len is not None else max(pos) + Sq
    pps = -(-cap // PAGE) + 1
    owned = sum(-(-(p + Sq) // PAGE) for p in pos if p >= 0)
    num_pages = num_pages or owned + 4
    perm = torch.randperm(num_pages, generator=g).tolist()
    nan_page = perm.pop()
    q = torch.randn(B, H, Sq, 128, generator=g).to(torch.bfloat16)
    kp = torch.full((num_pages, Hkv, PAGE, 128), 0x7F, dtype=torch.uint8)
    vp = kp.clone()
    ks = torch.full((num_pages, Hkv, PAGE), float("nan"))
    vs = ks.clone()
    table = torch.full((B, pps), nan_page, dtype=torch.int32)
    rows = []
    for b, p in enumerate(pos):
        if p < 0:
            rows.append(None)
            continue
        n = p + Sq
        k, v = _spread_rows(g, Hkv, n), _spread_rows(g, Hkv, n)
        k[0, n // 2] = 0                # zero bytes, scale 0, still visible
        rows.append((_requant(k), _requant(v)))
        (kq, ksc), (vq, vsc) = K.kv_quant_ref(k), K.kv_quant_ref(v)
        for j in range(-(-n // PAGE)):
            page = perm.pop()
            table[b, j] = page
            m = min(PAGE, n - j * PAGE)
            sl = slice(j * PAGE, j * PAGE + m)
            kp[page, :, :m], ks[page, :, :m] = kq[:, sl], ksc[:, sl]
            vp[page, :, :m], vs[page, :, :m] = vq[:, sl], vsc[:, sl]
    return q, [kp, vp, ks, vs], table, rows


def _run(dev, q, pool, table, pos, max_len):
    o = K.attn_append_paged_fp8(q.to(dev), *[t.to(dev) for t in pool],
                                table.to(dev), pos, SCALE, max_len=max_len)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    return o.float().cpu()


@pytest.mark.parametrize("B,H,Hkv,Sq,pos,max_len", SHAPES)
def test_matches_reference(dev, B, H, Hkv, Sq, pos, max_len):
    q, pool, table, rows = _fp8_case(B, H, Hkv, Sq, pos, max_len, seed=Sq)
    pos_t = torch.tensor(pos, dtype=torch.int32, device=dev)
    o = _run(dev, q, pool, table, pos_t, max_len)
    assert _check_rows(o, _reference(q, rows, pos),
                       "fp8 paged append %s" % (pos,)) < TOL


@pytest.mark.parametrize("B,H,Hkv,Sq,pos,holes", [
    (3, 4, 2, 5, [70, -1, 0], False),   # sequence 1 takes no part
    (2, 2, 1, 5, [150, 150], True),     # entry 1: -1, and past the pool
])
def test_skip_and_holes(dev, B, H, Hkv, Sq, pos, holes):
    q, pool, table, rows = _fp8_case(B, H, Hkv, Sq, pos, None, seed=2)
    num_pages = pool[0].size(0)
    if holes:
        table[0, 1], table[1, 1] = -1, num_pages
        refs = _reference(q, rows, pos, hidden=(PAGE, 2 * PAGE))
    else:
        table[1] = num_pages + 5        # never read
        refs = _reference(q, rows, pos)
    o = _run(dev, q, pool, table, pos, None)
    for b, p in enumerate(pos):
        if p < 0:
            assert bool((o[b] == 0).all()), "pos < 0 must give exact zeros"
    assert _check_rows(o, refs, "fp8 skip/holes %s" % (pos,)) < TOL


def test_slot_view_uses_the_kernel(dev, monkeypatch):
    from metaflow_amd.models.kv_cache import PagedKVCache
    from metaflow_amd.models.llama import LlamaConfig

    cfg = LlamaConfig.tiny(vocab=128, seq=256)
    H, Hkv = cfg.num_heads, cfg.num_kv_heads
    pc = PagedKVCache(cfg, 4, 2, 128, dev, dtype=torch.float8_e4m3fn)
    assert pc.reserve(2)
    pc.ensure(0, 1)                     # slot 1's page is not pool page 0
    pc.ensure(1, 47)
    pc.sync()
    for t in pc.k_pages + pc.v_pages:
        t.fill_(0x7F)
    for t in pc.k_scales + pc.v_scales:
        t.fill_(float("nan"))
    calls = []
    real = K.attn_append_paged_fp8
    monkeypatch.setattr(K, "attn_append_paged_fp8",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    monkeypatch.setattr(K, "kv_page_gather_fp8",
                        lambda *a, **kw: calls.append("gather"))
    g = torch.Generator().manual_seed(5)
    q = torch.randn(1, H, 47, 128, generator=g).to(torch.bfloat16)
    k, v = _spread_rows(g, 1, Hkv, 47), _spread_rows(g, 1, Hkv, 47)
    view = pc.slot_view(1)
    for lo, hi in ((0, 40), (40, 47)):
        view.pos = lo
        o = view.attend(0, q[:, :, lo:hi].to(dev), k[:, :, lo:hi].to(dev),
                        v[:, :, lo:hi].to(dev), hi - lo, SCALE)
    torch.cuda.synchronize()
    assert calls == [1]
    refs = _reference(q[:, :, 40:], [(_requant(k)[0], _requant(v)[0])], [40])
    assert _check_rows(o.float().cpu(), refs, "fp8 slot view") < TOL


def test_is_capturable(dev):
    """pos on the device and max_len the capacity: a captured call replayed
    after pos, q and the pool changed in place equals the eager call."""
    B, H, Hkv, Sq, cap = 2, 4, 2, 5, 1024          # 4 splits + the merge
    first = _fp8_case(B, H, Hkv, Sq, [300, 0], cap, seed=8, num_pages=24)
    second = _fp8_case(B, H, Hkv, Sq, [10, 500], cap, seed=9, num_pages=24)
    q, table = first[0].to(dev), first[2].to(dev)
    pool = [t.to(dev) for t in first[1]]
    pos_t = torch.tensor([300, 0], dtype=torch.int32, device=dev)

    def call():
        return K.attn_append_paged_fp8(q, *pool, table, pos_t, SCALE,
                                       max_len=cap)

    o_first = call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g = call()
    q.copy_(second[0])
    for dst, src in zip(pool, second[1]):
        dst.copy_(src)
    table.copy_(second[2])
    pos_t.copy_(torch.tensor([10, 500], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    o_e = call()
    torch.cuda.synchronize()
    assert not torch.isnan(o_g.float()).any()
    assert not torch.equal(o_g, o_first)        # the replay saw the change
    assert torch.equal(o_g, o_e)
