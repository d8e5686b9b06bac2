"""The FP8 paged KV cache on the GPU (decode_fp8.hip), by the method of
test_paged_gpu.py: unowned pages, rows past a length and the page stale
table entries point at hold the NaN byte 0x7F with NaN scales, pages are
shuffled, and rows carry per-row magnitudes over 2^+-6 so a wrong or shared
scale shows. Per row and head against fp32 attention_ref on the dequantised
rows at the kernel tolerance 2e-2 (fp32 up to the bf16 pack of P and the
store). Measured on an MI355X, worst row per decode shape: 3.1e-03,
3.5e-03, 3.6e-03, 3.6e-03 (docs/KERNELS.md, "FP8 paged decode")."""

import math

import pytest
import torch

from metaflow_amd.ops import kernels as K

from .test_paged_gpu import GRAPH_REQUESTS  # four page-crossing requests

pytestmark = pytest.mark.gpu

SCALE = 1.0 / math.sqrt(128)
TOL = 2e-2
PAGE = 64

# (B, H, Hkv, lengths, max_len)
DECODE_SHAPES = [
    (2, 4, 4, [1, 64], 64),             # G=1, one row, one exact page
    (2, 8, 2, [65, 200], 256),          # G=4, partial last page
    (3, 16, 2, [0, 129, 1000], 2048),   # G=8, inactive slot, empty splits
    (1, 32, 1, [130], 256),             # G=32, every B column real
]


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _spread_rows(g, *shape):
    """bf16 rows [..., 128], each with its own magnitude in 2^+-6."""
    mag = torch.exp2(12 * torch.rand(*shape, 1, generator=g) - 6)
    return (torch.randn(*shape, 128, generator=g) * mag).to(torch.bfloat16)


def fp8_case(B, H, Hkv, lengths, max_len, seed):
    """CPU: q, NaN-backed pools and scales, table, the original rows."""
    g = torch.Generator().manual_seed(seed)
    pps = -(-max_len // PAGE)
    num_pages = sum(-(-n // PAGE) for n in lengths) + 4
    perm = torch.randperm(num_pages, generator=g).tolist()
    nan_page = perm.pop()
    q = torch.randn(B, H, 1, 128, generator=g).to(torch.bfloat16)
    kp = torch.full((num_pages, Hkv, PAGE, 128), 0x7F, dtype=torch.uint8)
    vp = kp.clone()
    ks = torch.full((num_pages, Hkv, PAGE), float("nan"))
    vs = ks.clone()
    table = torch.full((B, pps), nan_page, dtype=torch.int32)
    rows = []
    for b, n in enumerate(lengths):
        k, v = _spread_rows(g, Hkv, n), _spread_rows(g, Hkv, n)
        rows.append((k, v))
        (kq, ksc), (vq, vsc) = K.kv_quant_ref(k), K.kv_quant_ref(v)
        for j in range(-(-n // PAGE)):
            page = perm.pop()
            table[b, j] = page
            m = min(PAGE, n - j * PAGE)
            sl = slice(j * PAGE, j * PAGE + m)
            kp[page, :, :m], ks[page, :, :m] = kq[:, sl], ksc[:, sl]
            vp[page, :, :m], vs[page, :, :m] = vq[:, sl], vsc[:, sl]
    return q, (kp, vp, ks, vs), table, rows


def _requant(x):
    return K.kv_dequant_ref(*K.kv_quant_ref(x))


def _row_err(o, ref):
    return ((o - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()


@pytest.mark.parametrize("B,H,Hkv,lengths,max_len", DECODE_SHAPES)
def test_attn_decode_paged_fp8_matches_reference(dev, B, H, Hkv, lengths,
                                                 max_len):
    q, pool, table, rows = fp8_case(B, H, Hkv, lengths, max_len, seed=7)
    o = K.attn_decode_paged_fp8(q.to(dev), *[t.to(dev) for t in pool],
                                table.to(dev), lengths, SCALE, max_len)
    torch.cuda.synchronize()
    o = o.float().cpu()
    worst = 0.0
    for b, n in enumerate(lengths):
        if n == 0:
            assert bool((o[b] == 0).all()), "inactive slot must be 0"
            continue
        k, v = rows[b]
        ref = K.attention_ref(q[b:b + 1].float(), _requant(k)[None],
                              _requant(v)[None], SCALE, causal=False)[0]
        assert not torch.isnan(ref).any()
        assert not torch.isnan(o[b]).any(), "read an unowned row or scale"
        worst = max(worst, _row_err(o[b], ref))
    print("fp8 paged decode %s worst row rel err %.3e" % (lengths, worst))
    assert worst < TOL


def _check_written(qb, scale, x, what):
    """Scales bit-equal to amax / 448, values within half an E4M3 step of
    x (the bound of test_kv_fp8.py); byte equality printed only."""
    xf = x.float()
    assert torch.equal(scale, xf.abs().amax(-1) / 448.0), what
    bound = 1.001 * torch.maximum(xf.abs() / 16, scale.unsqueeze(-1) / 1024)
    assert bool(((K.kv_dequant_ref(qb, scale) - xf).abs() <= bound).all()), \
        what
    same = (qb == K.kv_quant_ref(x)[0]).float().mean().item()
    print("%s: %.4f of the bytes equal kv_quant_ref's" % (what, same))


@pytest.mark.parametrize("S,pos", [(1, [0, 63, -1]), (70, [0, 60, 130])])
def test_kv_page_write_fp8(dev, S, pos):
    B, Hkv, num_pages, pps = 3, 2, 14, 4
    g = torch.Generator().manual_seed(11)
    table = torch.randperm(num_pages, generator=g)[:B * pps] \
        .view(B, pps).to(torch.int32)
    k, v = _spread_rows(g, B, Hkv, S), _spread_rows(g, B, Hkv, S)
    k[0, 0, 0] = 0  # a zero row: zero bytes, scale 0
    pools = [torch.full((num_pages, Hkv, PAGE, 128), 0x55, dtype=torch.uint8,
                        device=dev) for _ in range(2)]
    scales = [torch.full((num_pages, Hkv, PAGE), -7.0, device=dev)
              for _ in range(2)]
    # a strided V source (a slice of the QKV GEMM output)
    wide = torch.zeros(B, Hkv, S, 256, dtype=torch.bfloat16, device=dev)
    wide[..., 128:] = v.to(dev)
    K.kv_page_write_fp8(k.to(dev), wide[..., 128:], *pools, *scales,
                        table.to(dev),
                        torch.tensor(pos, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    written = torch.zeros(num_pages, Hkv, PAGE, dtype=torch.bool)
    for src, qb, sc in zip((k, v), [t.cpu() for t in pools],
                           [t.cpu() for t in scales]):
        for b, p in enumerate(pos):
            if p < 0:
                continue
            rows = torch.arange(p, p + S)
            pg, r = table[b, rows // PAGE].long(), rows % PAGE
            written[pg, :, r] = True
            _check_written(qb[pg, :, r], sc[pg, :, r],
                           src[b].transpose(0, 1), "S=%d b=%d" % (S, b))
        assert bool((qb[~written] == 0x55).all())
        assert bool((sc[~written] == -7.0).all())
    assert float(scales[0].cpu()[table[0, 0], 0, pos[0]]) == 0.0


def test_fp8_cache_decode_view(dev):
    """One decode_view(...).attend against attention_ref over the
    requantised old and new rows; the new row sits where the table says."""
    from metaflow_amd.models.kv_cache import PagedKVCache
    from metaflow_amd.models.llama import LlamaConfig

    cfg = LlamaConfig.tiny(vocab=128, seq=256)
    H, Hkv = cfg.num_heads, cfg.num_kv_heads
    positions = [5, 64, 130]
    B = len(positions)
    pc = PagedKVCache(cfg, 9, B, 256, dev, dtype=torch.float8_e4m3fn)
    assert pc.reserve(9)
    for rows in (1, 65, 129):  # interleaved: no slot's pages are contiguous
        for b, p in enumerate(positions):
            pc.ensure(b, min(rows, p + 1))
    pc.sync()
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, H, 1, 128, generator=g).to(torch.bfloat16)
    old = [(_spread_rows(g, 1, Hkv, p), _spread_rows(g, 1, Hkv, p))
           for p in positions]
    new_k, new_v = _spread_rows(g, B, Hkv, 1), _spread_rows(g, B, Hkv, 1)
    for t in pc.k_pages + pc.v_pages:
        t.fill_(0x7F)
    for t in pc.k_scales + pc.v_scales:
        t.fill_(float("nan"))
    for b, (k, v) in enumerate(old):
        K.kv_page_write_fp8(k.to(dev), v.to(dev), pc.k_pages[0],
                            pc.v_pages[0], pc.k_scales[0], pc.v_scales[0],
                            pc.block_table[b:b + 1], [0])
    view = pc.decode_view(positions, dev, 256)
    o = view.attend(0, q.to(dev), new_k.to(dev), new_v.to(dev), 1, SCALE)
    torch.cuda.synchronize()
    o = o.float().cpu()
    assert not torch.isnan(o).any()
    kp, ks = pc.k_pages[0].cpu(), pc.k_scales[0].cpu()
    for b, p in enumerate(positions):
        k_all = torch.cat([old[b][0], new_k[b:b + 1]], 2)
        v_all = torch.cat([old[b][1], new_v[b:b + 1]], 2)
        ref = K.attention_ref(q[b:b + 1].float(), _requant(k_all),
                              _requant(v_all), SCALE, causal=False)
        err = _row_err(o[b:b + 1], ref)
        print("fp8 decode view pos %d worst row rel err %.3e" % (p, err))
        assert err < TOL
        page = int(pc.table_host[b, p // PAGE])
        _check_written(kp[page, :, p % PAGE], ks[page, :, p % PAGE],
                       new_k[b, :, 0], "new row b=%d" % b)


def test_fp8_engine_graph_matches_eager(dev):
    from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from metaflow_amd.serving import ContinuousBatcher

    torch.manual_seed(0)
    model = LlamaForCausalLM(
        LlamaConfig.tiny(vocab=128, seq=256)).to(dev).eval()
    outs = []
    # graph replay, eager, eager with chunked prefill (gather stop-gap)
    for graph, chunk in ((True, None), (False, None), (False, 32)):
        b = ContinuousBatcher(model, max_batch=3, max_len=128, graph=graph,
                              num_pages=5, prefill_chunk=chunk,
                              kv_dtype=torch.float8_e4m3fn)
        assert b.cache.fp8 and (b._graph is not None) == graph
        reqs = [b.submit(p, n) for p, n in GRAPH_REQUESTS]
        res = b.run()
        outs.append([res[r.id] for r in reqs])
        assert b.cache.free_pages == 5
        assert bool((b.cache.table_host == -1).all())
    for run in outs:
        for toks, (_p, n) in zip(run, GRAPH_REQUESTS):
            assert len(toks) == n and all(0 <= t < 128 for t in toks)
    # graph replay and eager launch the same grids: identical tokens
    assert outs[0] == outs[1]
