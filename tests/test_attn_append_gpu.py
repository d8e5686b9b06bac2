"""append.hip on the GPU: K.attn_append against the fp32 reference on the
shapes that take each of the kernel's paths, and the model wiring.

The cache lives inside a larger NaN-filled allocation and every row past
pos+Sq is NaN, so an out-of-range read shows as a numerical failure, not
a fault. The check is PER ROW: one wrongly visible or hidden key at a
horizon <= 1000 moves its row by >= 3e-2, which a whole-tensor norm would
hide. 2e-2 is the project's kernel tolerance (test_ops_gpu.py); a CPU
emulation of the tilewise bf16-P algorithm on these shapes has a worst
per-row error of about 3e-3.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 1.0 / math.sqrt(128)
TOL = 2e-2

# (B, H, Hkv, Sq, pos, Lmax, max_len)
SHAPES = [
    # verify block, 1-wave kernel; pos+Sq == Lmax with Lmax % 64 != 0 (the
    # last tile straddles the allocation end); one sequence at pos 0
    (2, 4, 2, 5, [300, 0], 305, None),
    # 4-wave kernel; second query tile holds 2 of 128 rows; G = 4; pos
    # differs per sequence
    (2, 8, 2, 130, [0, 191], 342, None),
    # split count from the capacity: most rows see nothing in the later
    # splits (the -inf - -inf guard)
    (1, 2, 1, 128, [3], 2048, 2048),
    # long prefix, several non-empty splits, the merge
    (1, 2, 1, 64, [1000], 2048, 2048),
]


def setup_module():
    from metaflow_amd.ops import kernels as K

    assert K.extension_loaded(), "_mfx_hip must be built for GPU tests"


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _case(B, H, Hkv, Sq, pos, Lmax, seed):
    """CPU tensors: q, and NaN-backed caches with rows 0..pos+Sq-1 real."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Sq, 128, generator=g).to(torch.bfloat16)
    bigs = []
    for _ in range(2):
        big = torch.full((B + 1, Hkv, Lmax, 128), float("nan"),
                         dtype=torch.bfloat16)
        for b in range(B):
            n = pos[b] + Sq
            big[b, :, :n] = torch.randn(Hkv, n, 128, generator=g).to(
                torch.bfloat16)
        bigs.append(big)
    return q, bigs[0], bigs[1]


@pytest.mark.parametrize("B,H,Hkv,Sq,pos,Lmax,max_len", SHAPES)
def test_attn_append_matches_reference(dev, B, H, Hkv, Sq, pos, Lmax,
                                       max_len):
    from metaflow_amd.ops import kernels as K

    q, bigk, bigv = _case(B, H, Hkv, Sq, pos, Lmax, seed=Sq)
    ref = K.attn_append_ref(q, bigk[:B], bigv[:B], pos, SCALE).float()
    assert not torch.isnan(ref).any()

    gk, gv = bigk.to(dev), bigv.to(dev)
    pos_t = torch.tensor(pos, dtype=torch.int32, device=dev)
    o = K.attn_append(q.to(dev), gk[:B], gv[:B], pos_t, SCALE,
                      max_len=max_len)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == torch.bfloat16
    o = o.float().cpu()
    assert not torch.isnan(o).any(), "NaN in the output"
    err = (o - ref).norm(dim=-1) / ref.norm(dim=-1)       # [B, H, Sq]
    worst = err.max().item()
    print("worst per-row rel err %.3e at (b,h,i)=%s" % (
        worst, tuple((err == err.max()).nonzero()[0].tolist())))
    assert worst < TOL


def test_attn_append_int_and_list_pos(dev):
    """An int pos and a list take the same kernel path as the tensor."""
    from metaflow_amd.ops import kernels as K

    B, H, Hkv, Sq, Lmax = 2, 4, 2, 5, 128
    q, bigk, bigv = _case(B, H, Hkv, Sq, [70, 70], Lmax, seed=1)
    gq, gk, gv = q.to(dev), bigk.to(dev)[:B], bigv.to(dev)[:B]
    o_int = K.attn_append(gq, gk, gv, 70, SCALE)
    o_list = K.attn_append(gq, gk, gv, [70, 70], SCALE)
    o_t = K.attn_append(gq, gk, gv, torch.tensor([70, 70], device=dev),
                        SCALE, max_len=Lmax)
    ref = K.attn_append_ref(q, bigk[:B], bigv[:B], 70, SCALE).float()
    for o in (o_int, o_list, o_t):
        o = o.float().cpu()
        err = (o - ref).norm(dim=-1) / ref.norm(dim=-1)
        assert not torch.isnan(o).any() and err.max().item() < TOL


def _rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-8)).item()


def _wiring(model, cfg, dev, monkeypatch):
    from metaflow_amd.models.llama import KVCache
    from metaflow_amd.ops import kernels as K

    calls = []
    real = K.attn_append

    def counted(*a, **kw):
        calls.append(a[0].shape)
        return real(*a, **kw)

    monkeypatch.setattr(K, "attn_append", counted)
    g = torch.Generator().manual_seed(0)
    tokens = torch.randint(0, cfg.vocab_size, (1, 47), generator=g).to(dev)
    with torch.no_grad():
        full = model(tokens)
        cache = KVCache(cfg, 1, 64, dev)
        model(tokens[:, :40], cache=cache)
        assert calls == []          # prefill at pos 0 is the flash kernel
        block = model(tokens[:, 40:], cache=cache)
    torch.cuda.synchronize()
    assert len(calls) == cfg.num_layers
    assert all(s[2] == 7 for s in calls)
    assert cache.pos == 47
    assert not torch.isnan(block.float()).any()
    assert full[:, 40:47].float().abs().max() > 0     # not a 0 == 0 match
    err = _rel_err(block, full[:, 40:47])
    print("block vs uncached logits rel err %.3e" % err)
    assert err < TOL


def test_llama_cached_block_uses_append_kernel(dev, monkeypatch):
    from metaflow_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig.tiny(vocab=128, seq=256)
    model = LlamaForCausalLM(cfg).to(dev).eval()
    _wiring(model, cfg, dev, monkeypatch)


def test_mixtral_cached_block_uses_append_kernel(dev, monkeypatch):
    from metaflow_amd.models.mixtral import (MixtralConfig,
                                             MixtralForCausalLM)

    torch.manual_seed(0)
    cfg = MixtralConfig.tiny(vocab=128, seq=256)
    model = MixtralForCausalLM(cfg).to(dev).eval()
    _wiring(model, cfg, dev, monkeypatch)
