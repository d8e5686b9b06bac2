"""CPU path of K.attn_append_paged_fp8: gather through the table,
dequantise, attn_append_ref; pos < 0 gives zeros."""

import math

import torch

from metaflow_amd.ops import kernels as K

SCALE = 1.0 / math.sqrt(128)


def test_cpu_path_matches_reference_on_dequantised_rows():
    B, H, Hkv, Sq, pps, num_pages = 4, 4, 2, 5, 4, 12
    pos = [0, 65, 130, -1]
    g = torch.Generator().manual_seed(0)
    table = torch.randperm(num_pages, generator=g).view(B - 1, pps) \
        .to(torch.int32)
    table = torch.cat([table, torch.full((1, pps), -1, dtype=torch.int32)])
    kp = torch.full((num_pages, Hkv, 64, 128), 0x7F, dtype=torch.uint8)
    vp = kp.clone()
    ks = torch.full((num_pages, Hkv, 64), float("nan"))
    vs = ks.clone()
    q = torch.randn(B, H, Sq, 128, generator=g).to(torch.bfloat16)
    k = torch.randn(B, Hkv, 135, 128, generator=g).to(torch.bfloat16)
    v = torch.randn(B, Hkv, 135, 128, generator=g).to(torch.bfloat16)
    # the cache rows 0 .. pos+Sq-1 of each sequence, through the CPU write
    for b, p in enumerate(pos):
        if p >= 0:
            K.kv_page_write_fp8(k[b:b + 1, :, :p + Sq], v[b:b + 1, :, :p + Sq],
                                kp, vp, ks, vs, table[b:b + 1], [0])
    o = K.attn_append_paged_fp8(q, kp, vp, ks, vs, table, pos, SCALE)
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    assert bool((o[3] == 0).all())
    for b, p in enumerate(pos[:3]):
        n = p + Sq
        kd = K.kv_dequant_ref(*K.kv_quant_ref(k[b:b + 1, :, :n]))
        vd = K.kv_dequant_ref(*K.kv_quant_ref(v[b:b + 1, :, :n]))
        assert torch.equal(o[b:b + 1],
                           K.attn_append_ref(q[b:b + 1], kd, vd, p, SCALE))
