"""The FP8 paged KV cache off the GPU: the row format (K.kv_quant_ref /
K.kv_dequant_ref), the CPU path of K.attn_decode_paged_fp8, the cache's
allocation and the engine's argument check."""

import math

import pytest
import torch

from metaflow_amd.ops import kernels as K

SCALE = 1.0 / math.sqrt(128)


def test_kv_quant_bound():
    # magnitudes over 2^+-6, an all-zero row, a row with one 1e4 outlier
    g = torch.Generator().manual_seed(5)
    x = torch.randn(40, 128, generator=g)
    x = x * torch.exp2(torch.linspace(-6, 6, 40)).unsqueeze(-1)
    x[7] = 0
    x[11, 3] = 1e4
    x = x.to(torch.bfloat16)
    qb, scale = K.kv_quant_ref(x)
    assert qb.dtype == torch.uint8 and scale.dtype == torch.float32
    assert torch.equal(scale, x.float().abs().amax(-1) / 448.0)
    assert bool((qb[7] == 0).all()) and float(scale[7]) == 0.0
    # half an E4M3 step of x / scale: 2^-4 relative on normals (3 mantissa
    # bits), 2^-10 absolute on subnormals (step 2^-9), times scale
    deq = K.kv_dequant_ref(qb, scale)
    xf = x.float()
    bound = 1.001 * torch.maximum(xf.abs() / 16, scale.unsqueeze(-1) / 1024)
    assert bool(((deq - xf).abs() <= bound).all())


def test_attn_decode_paged_fp8_cpu_path():
    B, H, Hkv, lengths = 3, 4, 2, [0, 65, 130]
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, H, 1, 128, generator=g).to(torch.bfloat16)
    kp = torch.full((8, Hkv, 64, 128), 0x7F, dtype=torch.uint8)
    vp = kp.clone()
    ks = torch.full((8, Hkv, 64), float("nan"))
    vs = ks.clone()
    table = torch.tensor([[7, 7, 7], [5, 2, 7], [0, 6, 3]], dtype=torch.int32)
    pos = [-1, 0, 0]
    k = torch.randn(B, Hkv, 130, 128, generator=g).to(torch.bfloat16)
    v = torch.randn(B, Hkv, 130, 128, generator=g).to(torch.bfloat16)
    K.kv_page_write_fp8(k, v, kp, vp, ks, vs, table, pos)
    o = K.attn_decode_paged_fp8(q, kp, vp, ks, vs, table, lengths, SCALE, 192)
    assert bool((o[0] == 0).all())
    for b in (1, 2):
        n = lengths[b]
        kd = K.kv_dequant_ref(*K.kv_quant_ref(k[b:b + 1, :, :n]))
        vd = K.kv_dequant_ref(*K.kv_quant_ref(v[b:b + 1, :, :n]))
        ref = K.attention_ref(q[b:b + 1], kd, vd, SCALE, causal=False)
        assert torch.equal(o[b:b + 1], ref)
        assert torch.equal(K.kv_page_gather_fp8(kp, ks, table[b], n),
                           kd.to(torch.bfloat16))


def test_paged_cache_fp8_allocation():
    from metaflow_amd.models.kv_cache import PagedKVCache
    from metaflow_amd.models.llama import LlamaConfig

    cfg = LlamaConfig.tiny(vocab=128, seq=256)
    pc = PagedKVCache(cfg, 6, 2, 256, "cpu", dtype=torch.float8_e4m3fn)
    assert pc.fp8 and len(pc.k_pages) == cfg.num_layers
    for pages, scales in ((pc.k_pages, pc.k_scales),
                          (pc.v_pages, pc.v_scales)):
        for p, s in zip(pages, scales):
            assert p.dtype == torch.uint8
            assert p.numel() * p.element_size() \
                == 6 * cfg.num_kv_heads * 64 * 128
            assert s.dtype == torch.float32
            assert tuple(s.shape) == (6, cfg.num_kv_heads, 64)
    bf = PagedKVCache(cfg, 6, 2, 256, "cpu")
    assert not bf.fp8 and bf.k_pages[0].dtype == torch.bfloat16
    assert not hasattr(bf, "k_scales")


def test_engine_kv_dtype_needs_pages():
    from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from metaflow_amd.serving import ContinuousBatcher

    m = LlamaForCausalLM(LlamaConfig.tiny(vocab=128, seq=256))
    with pytest.raises(ValueError):
        ContinuousBatcher(m, max_batch=2, max_len=128, graph=False,
                          kv_dtype=torch.float8_e4m3fn)
