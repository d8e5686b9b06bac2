"""Exact-integer checks of the forward and the dQ kernel.

Both kernels feed an accumulator tile (P, dS) to their second MFMA as the
B operand of a transposed product, after a half exchange between the lane
halves that puts its rows in natural k order; the transposed reads of V
and K must supply the same rows in the same k slots, and the epilogue
transposes the result back through LDS. A wrong pairing or a wrong
transpose corrupts almost every element. With crafted inputs both results
are exact expressions, so the comparison is torch.equal, not a tolerance.

Forward (non-causal, scale = 0.125). Keys and queries carry a class in
{0, 1}: k[kv] = -64 e_g(kv), q[i] = 64 e_f(i). A score is -512 where the
classes match and 0 where they differ; exp(-512) underflows to exactly 0,
so P is 0 or 1 in a data-dependent pattern. Each class holds exactly S/2
keys at permuted positions, so l = S/2 is a power of two and

  O[i] = (sum over kv with g(kv) != f(i) of V[kv]) / (S/2),  lse = log(S/2)

with V sparse in {-1, 0, 1}. In kv head 0 the first 64-key tile is all
class 0, so class-0 queries of its heads see only matching keys there and
their next tile rescales the accumulator by exactly 0.

dQ (causal and not). q = 0, o = 0, lse = 0 give S = 0, P = 1 wherever
visible and delta = 0; with K, V and dO sparse in {-1, 0, 1}

  dQ = 0.125 * ((dO . V^T) o vis) . K,   dK = 0.

The tests assert, before they call a kernel, that every sum is below 256
in magnitude and that every expected output is exactly representable in
bf16.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 0.125
DENSITY = 0.1
SHAPES = [(1, 4, 2, 256), (2, 8, 2, 512)]


def _sparse(gen, *shape):
    keep = torch.rand(*shape, generator=gen) < DENSITY
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (keep * sign).to(torch.float64)


def _bf16_exact(x):
    return torch.equal(x.to(torch.bfloat16).to(torch.float64), x)


def _key_classes(gen, B, Hkv, S):
    """g[b, hk, kv] in {0, 1}, S/2 of each at permuted positions; kv head 0
    starts with 64 keys of class 0."""
    g = torch.empty(B, Hkv, S, dtype=torch.int64)
    for b in range(B):
        for hk in range(Hkv):
            if hk == 0:
                rest = torch.cat([torch.zeros(S // 2 - 64, dtype=torch.int64),
                                  torch.ones(S // 2, dtype=torch.int64)])
                rest = rest[torch.randperm(S - 64, generator=gen)]
                g[b, hk] = torch.cat([torch.zeros(64, dtype=torch.int64),
                                      rest])
            else:
                half = torch.arange(S) % 2
                g[b, hk] = half[torch.randperm(S, generator=gen)]
    assert bool((g.sum(-1) == S // 2).all())
    return g


@pytest.mark.parametrize("shape", SHAPES)
def test_fwd_exact(shape):
    from metaflow_amd.ops.kernels import hip_ext

    B, H, Hkv, S = shape
    G = H // Hkv
    gen = torch.Generator().manual_seed(11 + S)
    g = _key_classes(gen, B, Hkv, S)                       # [B,Hkv,S]
    f = torch.randint(0, 2, (B, H, S), generator=gen)      # [B,H,S]
    k = torch.zeros(B, Hkv, S, 128, dtype=torch.float64)
    k.scatter_(-1, g.unsqueeze(-1), -64.0)
    q = torch.zeros(B, H, S, 128, dtype=torch.float64)
    q.scatter_(-1, f.unsqueeze(-1), 64.0)
    v = _sparse(gen, B, Hkv, S, 128)

    gexp = g.repeat_interleave(G, dim=1)                   # [B,H,S]
    p = (f.unsqueeze(-1) != gexp.unsqueeze(-2)).to(torch.float64)
    assert bool((p.sum(-1) == S // 2).all())
    # class-0 queries of kv head 0's heads see no key in the first tile
    assert bool((p[:, :G, :, :64].sum(-1) == 0).any())
    sums = torch.matmul(p, v.repeat_interleave(G, dim=1))  # [B,H,S,128]
    assert sums.abs().max().item() < 256
    o_exp = sums / (S // 2)
    assert _bf16_exact(o_exp) and o_exp.abs().max().item() > 0

    dev = torch.device("cuda:0")
    bf = lambda t: t.to(torch.bfloat16).to(dev)
    o, lse = hip_ext().attn_fwd(bf(q), bf(k), bf(v), SCALE, False)
    assert torch.equal(o.cpu(), o_exp.to(torch.bfloat16)), "O"
    lse_err = (lse.cpu() - math.log(S // 2)).abs().max().item()
    print(shape, "lse max abs err", lse_err)
    assert lse_err < 1e-5, lse_err


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_dq_exact(shape, causal):
    from metaflow_amd.ops.kernels import hip_ext

    B, H, Hkv, S = shape
    G = H // Hkv
    gen = torch.Generator().manual_seed(23 + S)
    k = _sparse(gen, B, Hkv, S, 128)
    v = _sparse(gen, B, Hkv, S, 128)
    dout = _sparse(gen, B, H, S, 128)

    vis = torch.ones(S, S, dtype=torch.float64)            # [q, kv]
    if causal:
        vis = vis.tril()
    dp = torch.matmul(dout, v.repeat_interleave(G, dim=1)
                      .transpose(-1, -2)) * vis            # [B,H,q,kv]
    assert dp.abs().max().item() < 256
    dq_exp = torch.matmul(dp, k.repeat_interleave(G, dim=1)) * SCALE
    assert _bf16_exact(dq_exp) and dq_exp.abs().max().item() > 0

    dev = torch.device("cuda:0")
    bf = lambda t: t.to(torch.bfloat16).to(dev)
    kd, vd, dd = bf(k), bf(v), bf(dout)
    qd = torch.zeros_like(dd)
    od = torch.zeros_like(dd)
    lse = torch.zeros(B, H, S, dtype=torch.float32, device=dev)
    dq, dk, dv = hip_ext().attn_bwd(qd, kd, vd, od, dd, lse, SCALE, causal)
    assert torch.equal(dq.cpu(), dq_exp.to(torch.bfloat16)), "dQ"
    assert torch.equal(dk.cpu(), torch.zeros_like(kd).cpu()), "dK"
